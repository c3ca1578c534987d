// Host side of one divide-and-conquer merge (dc_merge.hh): the device block
// of a merge's vectors, the launches of kernels/dc_merge.hip, and the host
// twins of those kernels for the host target and the CPU tests.  All merge
// arithmetic is double.
//
// Device block of one merge (n sorted-basis entries, k active; DcMergeWork):
//   doubles: dd k | zz k | tau k | zh k | cs of every rotation list
//   ints:    org k | act k | defl n - k | ord n | inv_perm n | ab of every rotation list
#include "dc_merge.hh"

#include <algorithm>
#include <cmath>

namespace slate {
namespace internal {

namespace {

/// host twin of secular_roots + zhat
template <typename Poles>
void secular_host(Poles const& p, int64_t k, double rho, const double* z, double znorm2, int64_t* org, double* tau,
                  double* zh) {
    #pragma omp parallel for schedule(dynamic, 8) if (k > 64)
    for (int64_t j = 0; j < k; ++j) {
        int64_t o2 = j;
        tau[j] = secular::root_of<double>(p, k, j, rho, znorm2, &o2, [&](int64_t o, double t) {
            return secular::partial_sums<double>(p, k, j, z, o, t, 0, 1);
        });
        org[j] = o2;
    }
    #pragma omp parallel for schedule(static) if (k > 256)
    for (int64_t i = 0; i < k; ++i) zh[i] = secular::zhat_entry<double>(p, k, i, rho, z, org, tau);
}

/// host twin of merge_columns (the pointers of `a` and `rot` are host pointers)
template <typename R, typename Side>
void merge_columns_host(DcMerge const& a, DcRotations const& rot, Side const& side, int64_t ncols, R* M, int64_t ldm) {
    const int64_t rows = side.rows(a.n);
    const typename Side::Poles poles{a.dd};
    #pragma omp parallel for schedule(dynamic, 4)
    for (int64_t col = 0; col < ncols; ++col) {
        const int64_t jo = side.result(col);
        R* out = M + col * ldm;
        if (jo >= a.n) {
            for (int64_t r = 0; r < rows; ++r) out[r] = R(side.null_entry(r, a.n));
            continue;
        }
        std::vector<double> vec(size_t(a.n), 0.0);
        const int64_t r = a.ord[jo];
        if (r < a.k) {
            const double dr = a.dd[a.org[r]], tr = a.tau[r];
            double nrm = 0;
            for (int64_t i = 0; i < a.k; ++i) {
                const double u = side.entry(i, a.dd[i], a.zh[i] / poles.pole_minus_root(i, dr, tr));
                vec[a.act[i]] = u;
                nrm += u * u;
            }
            nrm = 1.0 / std::sqrt(nrm);
            for (int64_t i = 0; i < a.k; ++i) vec[a.act[i]] *= nrm;
        } else {
            vec[a.defl[r - a.k]] = 1.0;
        }
        // G w with G = G_1 ... G_t: the last rotation acts first
        for (int64_t t = rot.nrot - 1; t >= 0; --t) {
            const int64_t x = rot.ab[2 * t], y = rot.ab[2 * t + 1];
            const double c = rot.cs[2 * t], sn = rot.cs[2 * t + 1], vx = vec[x], vy = vec[y];
            vec[x] = c * vx - sn * vy;
            vec[y] = sn * vx + c * vy;
        }
        for (int64_t row = 0; row < rows; ++row) out[row] = R(side.row_entry(row, a.n, vec.data(), a.inv_perm));
    }
}

}  // namespace

bool close_pole_rotation(std::vector<double>& Ds, std::vector<double>& zs, int64_t last, int64_t s, double tol,
                         std::initializer_list<RotationList*> record) {
    const double t = std::hypot(zs[last], zs[s]);
    const double cc = zs[s] / t, sn = -zs[last] / t;
    if (!(std::abs((Ds[s] - Ds[last]) * cc * sn) <= tol)) return false;
    for (RotationList* r : record) {
        r->ab.push_back(last); r->ab.push_back(s);
        r->cs.push_back(cc); r->cs.push_back(sn);
    }
    const double dl = Ds[last], ds = Ds[s];
    Ds[last] = dl * cc * cc + ds * sn * sn;
    Ds[s] = dl * sn * sn + ds * cc * cc;
    zs[s] = t;
    zs[last] = 0;
    return true;
}

template <typename Poles>
void secular_solve(lb::Ctx const& c, DcMergeWork& ws, int64_t n, int64_t nrot, int64_t k, double rho,
                   std::vector<double> const& dd, std::vector<double> const& zz, double znorm2,
                   std::vector<int64_t>& org, std::vector<double>& tau, std::vector<double>& zh) {
    org.assign(k, 0);
    tau.assign(k, 0.0);
    if (!c.dev()) {
        zh.assign(k, 0.0);
        secular_host(Poles{dd.data()}, k, rho, zz.data(), znorm2, org.data(), tau.data(), zh.data());
        return;
    }
    zh.clear();
    ws.dvec.resize(Target::Devices, size_t(4 * k + 2 * nrot + 1));
    ws.divec.resize(Target::Devices, size_t(2 * k + 3 * n + 2 * nrot + 1));
    double* dv = ws.dvec.data();
    int64_t* iv = ws.divec.data();
    device::memcpy_async(dv, dd.data(), k * sizeof(double), c.stream);
    device::memcpy_async(dv + k, zz.data(), k * sizeof(double), c.stream);
    slate_amd::dev::secular_roots(Poles{dv}, k, rho, dv + k, znorm2, iv, dv + 2 * k, c.stream);
    slate_amd::dev::zhat(Poles{dv}, k, rho, dv + k, iv, dv + 2 * k, dv + 3 * k, c.stream);
    device::memcpy_async(org.data(), iv, k * sizeof(int64_t), c.stream);
    device::memcpy_async(tau.data(), dv + 2 * k, k * sizeof(double), c.stream);
    slate_hip_call(hipStreamSynchronize(c.stream));
}

DcMerge merge_layout(lb::Ctx const& c, DcMergeWork& ws, int64_t n, std::vector<double> const& dd,
                     std::vector<double> const& zh, std::vector<double> const& tau, std::vector<int64_t> const& org,
                     std::vector<int64_t> const& act, std::vector<int64_t> const& defl, std::vector<int64_t> const& ord,
                     std::vector<int64_t> const& inv_perm, std::initializer_list<RotationList const*> rots,
                     DcRotations* rot_out) {
    DcMerge mg;
    const int64_t k = int64_t(act.size());
    mg.n = n; mg.k = k;
    if (!c.dev()) {
        mg.dd = dd.data(); mg.zh = zh.data(); mg.tau = tau.data();
        mg.org = org.data(); mg.act = act.data(); mg.defl = defl.data(); mg.ord = ord.data();
        mg.inv_perm = inv_perm.data();
        for (RotationList const* r : rots) *rot_out++ = DcRotations{r->count(), r->ab.data(), r->cs.data()};
        return mg;
    }
    double* dv = ws.dvec.data();
    int64_t* iv = ws.divec.data();
    device::memcpy_async(iv + k, act.data(), k * sizeof(int64_t), c.stream);
    if (n > k) device::memcpy_async(iv + 2 * k, defl.data(), (n - k) * sizeof(int64_t), c.stream);
    device::memcpy_async(iv + k + n, ord.data(), n * sizeof(int64_t), c.stream);
    device::memcpy_async(iv + k + 2 * n, inv_perm.data(), n * sizeof(int64_t), c.stream);
    mg.dd = dv; mg.tau = dv + 2 * k; mg.zh = dv + 3 * k;
    mg.org = iv; mg.act = iv + k; mg.defl = iv + 2 * k; mg.ord = iv + k + n; mg.inv_perm = iv + k + 2 * n;
    int64_t at = 0;   // rotations before this list
    for (RotationList const* r : rots) {
        const int64_t nr = r->count();
        if (nr) {
            device::memcpy_async(iv + k + 3 * n + 2 * at, r->ab.data(), 2 * nr * sizeof(int64_t), c.stream);
            device::memcpy_async(dv + 4 * k + 2 * at, r->cs.data(), 2 * nr * sizeof(double), c.stream);
        }
        *rot_out++ = DcRotations{nr, iv + k + 3 * n + 2 * at, dv + 4 * k + 2 * at};
        at += nr;
    }
    return mg;
}

template <typename R, typename Side>
int64_t merge_columns(lb::Ctx const& c, DcMergeWork& ws, DcMerge const& mg, DcRotations const& rot, Side const& side,
                      int64_t ncols, R* M, int64_t ldm) {
    if (!c.dev()) {
        merge_columns_host<R>(mg, rot, side, ncols, M, ldm);
        return 0;
    }
    // columns in batches: scratch of batch x n doubles under a byte budget
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(ncols, int64_t(256 << 20) / (8 * std::max<int64_t>(mg.n, 1))));
    ws.dscr.resize(Target::Devices, size_t(batch) * mg.n);
    int64_t launches = 0;
    for (int64_t c0 = 0; c0 < ncols; c0 += batch, ++launches)
        slate_amd::dev::merge_columns<R>(mg, rot, side, c0, std::min(batch, ncols - c0), M, ldm, ws.dscr.data(),
                                         c.stream);
    return launches;
}

#define SLATE_DC_SOLVE_INST(P)                                                                                   \
    template void secular_solve<P>(lb::Ctx const&, DcMergeWork&, int64_t, int64_t, int64_t, double,              \
                                   std::vector<double> const&, std::vector<double> const&, double,               \
                                   std::vector<int64_t>&, std::vector<double>&, std::vector<double>&);
SLATE_DC_SOLVE_INST(secular::LinearPoles<double>)
SLATE_DC_SOLVE_INST(secular::SquaredPoles<double>)
#define SLATE_DC_COLUMNS_INST(R, S)                                                                               \
    template int64_t merge_columns<R, S>(lb::Ctx const&, DcMergeWork&, DcMerge const&, DcRotations const&, S const&, \
                                         int64_t, R*, int64_t);
SLATE_DC_COLUMNS_INST(float, StedcSide)
SLATE_DC_COLUMNS_INST(double, StedcSide)
SLATE_DC_COLUMNS_INST(float, BdsdcSide)
SLATE_DC_COLUMNS_INST(double, BdsdcSide)

}  // namespace internal
}  // namespace slate
