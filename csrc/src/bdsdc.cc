// Bidiagonal divide and conquer (Gu-Eisenstat; the structure of LAPACK's
// bdsdc / lasd0 .. lasd8, written from the math): singular values and both
// vector sets of an upper bidiagonal B (d, e), B = U_B diag(sigma) V_B^T.
//
// Replicated compute.  Unlike stedc_dist (eig_dist.cc) the children of a node
// are offset by one row (U1 is NL x NL, then the removed row, then U2), which
// does not follow tile boundaries; so every process runs the whole divide and
// conquer on LOCAL contiguous column-major arrays -- U_B, V_B, one work array
// and one merge matrix, about 4 n^2 reals per process, in device memory on
// the device target and in host memory on the host target -- with the same
// input, the same kernels and no communication, and keeps what it owns.
//
// A node is an N x (N + sqre) block.  Removing row k (alpha = d_k,
// beta = e_k) leaves B1 (NL x (NL + 1), sqre 1) and B2 (NR x (NR + sqre));
// with B1 = U1 [D1 0] V1^T, B2 = U2 [D2 (0)] V2^T, l1 / lambda1 the last row
// of V1, f2 / phi2 the first row of V2 and one rotation of the null vectors
// (q1, q2) with r0 = hypot(alpha lambda1, beta phi2), the middle matrix is
//   M = [ z^T ; 0 diag(d_2 .. d_N) ],  z = (r0, alpha l1, beta f2), d_1 = 0.
// Host, O(N): sort, three deflations (|z_i| tiny; d_i tiny: z_i rotated into
// z_1 on the V side; two close d: one z rotated away on both sides; rotations
// recorded, not applied).  Then the merge shared with stedc_dist (dc_merge.hh;
// device kernels/dc_merge.hip, host twins dc_merge.cc) on the poles d_i^2:
// secular roots, z recomputed from the roots, the merge matrices MU / MV.
// Then U := diag(U1, 1, U2) MU and V := diag(V1, V2) MV, two GEMMs each on
// the local MFMA GEMM.  Leaves (<= SLATE_BDSDC_LEAF rows, default 64) run
// host::bdsqr; a sqre = 1 leaf first chases its extra column away with Givens
// rotations from the right.  All secular arithmetic is double, also for float.
//
// Accuracy is absolute (eps ||B||): tiny singular values do not get the
// relative accuracy of the QR iteration.
#include "internal.hh"
#include "dc_merge.hh"
#include "slate_amd/eig_host.hh"
#include "../kernels/kernels.hh"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <numeric>

namespace slate {
namespace internal {

namespace {

std::mutex g_stats_mu;
BdsdcStats g_stats;   // of the last call in this process

int64_t leaf_size() {
    const char* e = std::getenv("SLATE_BDSDC_LEAF");
    return std::max<int64_t>(2, e ? std::atoll(e) : 64);
}

using slate_amd::dev::BdsdcPlace;

template <typename R>
struct Solver {
    lb::Ctx c;
    int64_t n = 0, ld = 0, leaf = 64;
    std::vector<double> d, e;            // scaled bidiagonal; d becomes sigma block by block
    R *U = nullptr, *V = nullptr, *W = nullptr, *M = nullptr;
    BdsdcStats st;
    DcMergeWork ws;

    void sync() { if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream)); }

    /// dense host block (m x m, ld m) into dst (ld)
    void put(std::vector<R> const& src, int64_t m, R* dst) {
        if (c.dev()) {
            device::memcpy2d_async(dst, ld * sizeof(R), src.data(), m * sizeof(R), m * sizeof(R), m, c.stream);
            sync();
        } else {
            for (int64_t j = 0; j < m; ++j) std::copy(src.begin() + j * m, src.begin() + (j + 1) * m, dst + j * ld);
        }
    }

    /// cnt entries of a row (stride ld) to the host
    void row(const R* src, int64_t cnt, double* out) {
        if (cnt <= 0) return;
        std::vector<R> h(cnt);
        if (c.dev()) {
            device::memcpy2d_async(h.data(), sizeof(R), src, ld * sizeof(R), sizeof(R), cnt, c.stream);
            sync();
        } else {
            for (int64_t t = 0; t < cnt; ++t) h[t] = src[t * ld];
        }
        for (int64_t t = 0; t < cnt; ++t) out[t] = double(h[t]);
    }

    void solve(int64_t lo, int64_t N, int64_t sqre, int depth) {
        if (N <= leaf) { leaf_solve(lo, N, sqre); return; }
        const int64_t NL = N / 2, NR = N - NL - 1;
        solve(lo, NL, 1, depth + 1);
        solve(lo + NL + 1, NR, sqre, depth + 1);
        merge(lo, N, sqre, NL, depth);
    }

    /// m x (m + sqre) leaf on the host: U block m x m, V block (m + sqre) square
    void leaf_solve(int64_t lo, int64_t m, int64_t sqre) {
        trace::Block tb("bdsdc_leaves");
        std::vector<double> dl(d.begin() + lo, d.begin() + lo + m), el(std::max<int64_t>(m - 1, 0));
        for (int64_t i = 0; i + 1 < m; ++i) el[i] = e[lo + i];
        const int64_t mv = m + sqre;
        // sqre = 1: B G_{m-1} ... G_0 = [B' 0], G_i on columns (i, m)
        std::vector<double> gc, gs;
        if (sqre) {
            gc.resize(m); gs.resize(m);
            double x = e[lo + m - 1];
            for (int64_t i = m - 1; i >= 0; --i) {
                const double r = std::hypot(dl[i], x);
                const double cc = r == 0 ? 1.0 : dl[i] / r, sn = r == 0 ? 0.0 : x / r;
                dl[i] = r;
                gc[i] = cc; gs[i] = sn;
                if (i > 0) { x = -sn * el[i - 1]; el[i - 1] = cc * el[i - 1]; }
            }
        }
        std::vector<double> Ul(size_t(m) * m, 0.0), VTl(size_t(m) * m, 0.0);
        for (int64_t i = 0; i < m; ++i) { Ul[i + i * m] = 1; VTl[i + i * m] = 1; }
        const int64_t info = host::bdsqr<double, double>(m, dl.data(), el.data(), Ul.data(), m, m, VTl.data(), m, m);
        slate_error_if_msg(info != 0, "bdsdc: leaf QR iteration did not converge");
        // V = G_{m-1} ... G_0 diag(V', 1)
        std::vector<double> Vl(size_t(mv) * mv, 0.0);
        for (int64_t j = 0; j < m; ++j)
            for (int64_t i = 0; i < m; ++i) Vl[i + j * mv] = VTl[j + i * m];
        if (sqre) {
            Vl[m + m * mv] = 1;
            for (int64_t i = 0; i < m; ++i) {
                const double cc = gc[i], sn = gs[i];
                for (int64_t j = 0; j < mv; ++j) {
                    const double a = Vl[i + j * mv], b = Vl[m + j * mv];
                    Vl[i + j * mv] = cc * a - sn * b;
                    Vl[m + j * mv] = sn * a + cc * b;
                }
            }
        }
        std::vector<R> hu(Ul.begin(), Ul.end()), hv(Vl.begin(), Vl.end());
        put(hu, m, U + lo + lo * ld);
        put(hv, mv, V + lo + lo * ld);
        std::copy(dl.begin(), dl.end(), d.begin() + lo);
    }

    void merge(int64_t lo, int64_t N, int64_t sqre, int64_t NL, int depth) {
        const int64_t NR = N - NL - 1, kr = lo + NL, Nv = N + sqre;
        const double alpha = d[kr], beta = e[kr];
        const bool dev = c.dev();
        // ---- z, sort, deflation
        trace::Block t_defl("bdsdc_m_deflate");
        std::vector<double> z(N, 0.0), dn(N, 0.0);
        double lambda1 = 0, phi2 = 0;
        {
            std::vector<double> r1(NL + 1), r2(NR + sqre);
            row(V + kr + lo * ld, NL + 1, r1.data());
            row(V + (kr + 1) + (kr + 1) * ld, NR + sqre, r2.data());
            for (int64_t i = 0; i < NL; ++i) { z[i] = alpha * r1[i]; dn[i] = d[lo + i]; }
            for (int64_t i = 0; i < NR; ++i) { z[NL + 1 + i] = beta * r2[i]; dn[NL + 1 + i] = d[kr + 1 + i]; }
            lambda1 = r1[NL];
            if (sqre) phi2 = r2[NR];
        }
        const double r0 = std::hypot(alpha * lambda1, beta * phi2);
        const double qc = r0 == 0 ? 1.0 : alpha * lambda1 / r0, qs = r0 == 0 ? 0.0 : beta * phi2 / r0;
        z[NL] = r0;
        dn[NL] = 0;
        // sorted basis: the removed row first, then d ascending
        std::vector<int64_t> perm(N);
        perm[0] = NL;
        for (int64_t i = 0, s = 1; i < N; ++i) if (i != NL) perm[s++] = i;
        std::stable_sort(perm.begin() + 1, perm.end(), [&](int64_t a, int64_t b) { return dn[a] < dn[b]; });
        std::vector<double> Ds(N), zs(N);
        for (int64_t s = 0; s < N; ++s) { Ds[s] = dn[perm[s]]; zs[s] = z[perm[s]]; }
        std::vector<char> defl_flag(N, 0);
        RotationList rot_u, rot_v;
        {
            const double eps = std::numeric_limits<R>::epsilon();
            double dmax = 0, zmax = 0;
            for (int64_t s = 0; s < N; ++s) { dmax = std::max(dmax, std::abs(Ds[s])); zmax = std::max(zmax, std::abs(zs[s])); }
            const double tol = 8.0 * eps * std::max(dmax, zmax);
            int64_t last = -1;
            for (int64_t s = 1; s < N; ++s) {
                if (std::abs(zs[s]) <= tol) { zs[s] = 0; defl_flag[s] = 1; continue; }
                if (Ds[s] <= tol) {
                    // tiny d: z_s rotated into z_0 (V side only), a zero singular value
                    const double t = std::hypot(zs[0], zs[s]);
                    rot_v.ab.push_back(s); rot_v.ab.push_back(0);
                    rot_v.cs.push_back(zs[0] / t); rot_v.cs.push_back(-zs[s] / t);
                    zs[0] = t; zs[s] = 0; Ds[s] = 0;
                    defl_flag[s] = 1;
                    continue;
                }
                // close poles: one z rotated to zero on both sides
                if (last >= 0 && close_pole_rotation(Ds, zs, last, s, tol, {&rot_u, &rot_v})) defl_flag[last] = 1;
                last = s;
            }
            if (std::abs(zs[0]) <= tol) zs[0] = tol;
        }
        std::vector<int64_t> act, defl;
        for (int64_t s = 0; s < N; ++s) (defl_flag[s] ? defl : act).push_back(s);
        std::stable_sort(act.begin() + 1, act.end(), [&](int64_t a, int64_t b) { return Ds[a] < Ds[b]; });
        const int64_t k = int64_t(act.size());
        std::vector<double> dd(k), zz(k);
        double znorm2 = 0;
        for (int64_t i = 0; i < k; ++i) { dd[i] = Ds[act[i]]; zz[i] = zs[act[i]]; znorm2 += zz[i] * zz[i]; }
        t_defl.end();
        ++st.merges;
        st.columns += N;
        st.deflated += N - k;
        if (int64_t(st.level_columns.size()) <= depth) { st.level_columns.resize(depth + 1, 0); st.level_deflated.resize(depth + 1, 0); }
        st.level_columns[depth] += N;
        st.level_deflated[depth] += N - k;
        // ---- secular roots, z-hat
        std::vector<int64_t> org;
        std::vector<double> tau, zh;
        trace::Block t_sec("bdsdc_m_secular");
        secular_solve<secular::SquaredPoles<double>>(c, ws, N, rot_u.count() + rot_v.count(), k, 1.0, dd, zz, znorm2,
                                                     org, tau, zh);
        if (dev) {
            ++st.launches_secular;
            ++st.launches_zhat;
        }
        t_sec.end();
        // ---- singular values of the node, descending
        std::vector<double> sig(N);
        for (int64_t r = 0; r < k; ++r) sig[r] = dd[org[r]] + tau[r];
        for (int64_t t = 0; t < N - k; ++t) sig[k + t] = Ds[defl[t]];
        std::vector<int64_t> ord(N), inv_perm(N);
        std::iota(ord.begin(), ord.end(), int64_t(0));
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return sig[a] > sig[b]; });
        for (int64_t s = 0; s < N; ++s) inv_perm[perm[s]] = s;
        DcRotations drot[2];   // U side, V side
        DcMerge mg;
        {
            trace::Block t_m("bdsdc_m_matrix");
            mg = merge_layout(c, ws, N, dd, zh, tau, org, act, defl, ord, inv_perm, {&rot_u, &rot_v}, drot);
        }
        BdsdcSide side;
        side.nl = NL; side.sqre = sqre; side.qc = qc; side.qs = qs;
        auto build = [&](int vside) {
            trace::Block t_m("bdsdc_m_matrix");
            side.vside = vside;
            st.launches_matrix += merge_columns<R>(c, ws, mg, drot[vside], side, vside ? Nv : N, M, ld);
        };
        auto gemm_ = [&](int64_t mm, int64_t nn, int64_t kk, const R* A, const R* B, R* C) {
            if (mm > 0 && nn > 0 && kk > 0)
                lb::gemm<R>(c, Op::NoTrans, Op::NoTrans, mm, nn, kk, R(1), A, ld, B, ld, R(0), C, ld);
        };
        // ---- U := diag(U1, 1, U2) MU
        build(0);
        {
            trace::Block t_g("bdsdc_m_gemm");
            R* Ub = U + lo + lo * ld;
            gemm_(NL + 1, N, NL + 1, Ub, M, W);
            gemm_(NR, N, NR, Ub + (NL + 1) + (NL + 1) * ld, M + NL + 1, W + NL + 1);
            lb::copy2d(c, N, N, W, ld, Ub, ld);
        }
        // ---- V := diag(V1, V2) MV
        build(1);
        {
            trace::Block t_g("bdsdc_m_gemm");
            R* Vb = V + lo + lo * ld;
            gemm_(NL + 1, Nv, NL + 1, Vb, M, W);
            gemm_(NR + sqre, Nv, NR + sqre, Vb + (NL + 1) + (NL + 1) * ld, M + NL + 1, W + NL + 1);
            lb::copy2d(c, Nv, Nv, W, ld, Vb, ld);
            sync();   // the host vectors of this merge are done with
        }
        for (int64_t jo = 0; jo < N; ++jo) d[lo + jo] = sig[ord[jo]];
    }
};

}  // namespace

BdsdcStats bdsdc_stats_copy() {
    std::lock_guard<std::mutex> lk(g_stats_mu);
    return g_stats;
}

template <typename R>
void bdsdc_local(lb::Ctx const& c, std::vector<R>& D, std::vector<R> const& E, R* UB, R* VB, int64_t ld) {
    const int64_t n = int64_t(D.size());
    if (n == 0) return;
    slate_assert(ld >= n);
    const Target tg = c.dev() ? Target::Devices : Target::HostTask;
    Solver<R> s;
    s.c = c; s.n = n; s.ld = ld; s.leaf = leaf_size();
    s.U = UB; s.V = VB;
    s.d.assign(D.begin(), D.end());
    s.e.assign(n, 0.0);
    for (int64_t i = 0; i + 1 < n && i < int64_t(E.size()); ++i) s.e[i] = double(E[i]);
    // unit max-norm
    double smax = 0;
    for (int64_t i = 0; i < n; ++i) smax = std::max({smax, std::abs(s.d[i]), std::abs(s.e[i])});
    slate_error_if_msg(!std::isfinite(smax), "bdsdc: the bidiagonal has a NaN or Inf entry");
    // U starts as the identity: the removed row of every node is a unit row
    // until its merge, so diag(U1, 1) is one stored block
    lb::set(c, Uplo::General, n, n, R(0), R(1), UB, ld);
    lb::set(c, Uplo::General, n, n, R(0), R(smax == 0 ? 1 : 0), VB, ld);
    if (smax == 0) {
        if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
        std::fill(D.begin(), D.end(), R(0));
        return;
    }
    for (int64_t i = 0; i < n; ++i) { s.d[i] /= smax; s.e[i] /= smax; }
    Work<R> W(tg, size_t(ld) * n), M(tg, size_t(ld) * n);
    s.W = W.data(); s.M = M.data();
    // independent problems between exact zeros of e
    int64_t nseg = 0;
    for (int64_t s0 = 0; s0 < n;) {
        int64_t s1 = s0 + 1;
        while (s1 < n && s.e[s1 - 1] != 0) ++s1;
        s.solve(s0, s1 - s0, 0, 0);
        s0 = s1;
        ++nseg;
    }
    if (nseg > 1) {
        // blocks are descending one by one: one global order
        std::vector<int64_t> perm(n);
        std::iota(perm.begin(), perm.end(), int64_t(0));
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return s.d[a] > s.d[b]; });
        std::vector<double> ds(n);
        for (int64_t j = 0; j < n; ++j) ds[j] = s.d[perm[j]];
        s.d = ds;
        for (R* X : {UB, VB}) {
            for (int64_t j = 0; j < n; ++j) lb::copy2d(c, n, 1, X + perm[j] * ld, ld, s.W + j * ld, ld);
            lb::copy2d(c, n, n, s.W, ld, X, ld);
        }
    }
    if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
    for (int64_t i = 0; i < n; ++i) D[i] = R(s.d[i] * smax);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_stats = s.st;
}

template <typename T>
void bdsdc_place(lb::Ctx const& c, Matrix<T>& A, real_type<T> const* src, int64_t lds, bool trans,
                 std::vector<T> const& phase) {
    using R = real_type<T>;
    slate_error_if_msg(A.op() != Op::NoTrans || !A.aligned(), "bdsdc: placement needs a whole NoTrans matrix");
    LocalBlock<T> la = A.local(c.loc(), true);
    if (la.empty()) return;
    auto& st = *A.storage();
    auto& g = *A.grid();
    BdsdcPlace p;
    p.m = A.m(); p.n = A.n();
    p.lrows = la.m; p.lcols = la.n;
    p.mb = st.mb; p.p = g.p(); p.rrel = st.rrel();
    p.nb = st.nb; p.q = g.q(); p.crel = st.crel();
    p.trans = trans ? 1 : 0;
    if (c.dev()) {
        Work<T> ph;
        if (!phase.empty()) {
            ph.resize(Target::Devices, phase.size());
            device::memcpy_async(ph.data(), phase.data(), phase.size() * sizeof(T), c.stream);
        }
        slate_amd::dev::bdsdc_place(p, src, lds, phase.empty() ? nullptr : slate_amd::dev::dptr(ph.data()),
                                    slate_amd::dev::dptr(la.ptr), la.ld, c.stream);
        slate_hip_call(hipStreamSynchronize(c.stream));
        return;
    }
    #pragma omp parallel for schedule(static)
    for (int64_t lc = 0; lc < p.lcols; ++lc) {
        const int64_t gj = ((lc / p.nb) * p.q + p.crel) * p.nb + lc % p.nb;
        if (gj >= p.n) continue;
        for (int64_t lr = 0; lr < p.lrows; ++lr) {
            const int64_t gi = ((lr / p.mb) * p.p + p.rrel) * p.mb + lr % p.mb;
            if (gi >= p.m) continue;
            const R v = trans ? src[gj + gi * lds] : src[gi + gj * lds];
            la.ptr[lr + lc * la.ld] = phase.empty() ? T(v) : phase[gi] * v;
        }
    }
}

#define SLATE_BDSDC_PLACE_INST(T)                                                                          \
    template void bdsdc_place<T>(lb::Ctx const&, Matrix<T>&, real_type<T> const*, int64_t, bool, std::vector<T> const&);
SLATE_BDSDC_PLACE_INST(float)
SLATE_BDSDC_PLACE_INST(double)
SLATE_BDSDC_PLACE_INST(std::complex<float>)
SLATE_BDSDC_PLACE_INST(std::complex<double>)
template void bdsdc_local<float>(lb::Ctx const&, std::vector<float>&, std::vector<float> const&, float*, float*, int64_t);
template void bdsdc_local<double>(lb::Ctx const&, std::vector<double>&, std::vector<double> const&, double*, double*,
                                  int64_t);

}  // namespace internal

BdsdcStats bdsdc_stats() { return internal::bdsdc_stats_copy(); }

//------------------------------------------------------------------------------
template <typename T>
void bdsdc(Job jobu, Job jobvt, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E, Matrix<T>& U,
           Matrix<T>& VT, Options const& opts) {
    trace::Block tb("bdsdc");
    internal::DriverScope ds_;
    using R = real_type<T>;
    const int64_t n = int64_t(D.size());
    const bool wu = jobu != Job::NoVec && U.m() > 0 && U.n() > 0, wv = jobvt != Job::NoVec && VT.m() > 0 && VT.n() > 0;
    if (!wu && !wv) {
        // values only: O(n^2) on the host, no divide and conquer
        int64_t info = host::bdsqr_core<R>(n, D.data(), E.data(), nullptr);
        slate_error_if_msg(info != 0, "bdsdc: QR iteration did not converge");
        return;
    }
    slate_error_if_msg((wu && U.n() != n) || (wv && VT.m() != n), "bdsdc: U must be m x n and VT n x n");
    if (n == 0) return;
    const Target target = internal::resolve_target(opts);
    lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
    internal::Work<R> UB(target, size_t(n) * n), VB(target, size_t(n) * n);
    internal::bdsdc_local<R>(c, D, E, UB.data(), VB.data(), n);
    const std::vector<T> no_phase;
    if (wu) {
        // U := U U_B
        const int64_t b = std::max<int64_t>(1, U.nb());
        Matrix<T> Ub(n, n, b, b, U.grid()), Uo(U.m(), n, std::max<int64_t>(1, U.mb()), b, U.grid());
        Ub.insertLocalTiles(target);
        Uo.insertLocalTiles(target);
        internal::bdsdc_place<T>(c, Ub, UB.data(), n, false, no_phase);
        gemm(T(1), U, Ub, T(0), Uo, opts);
        slate::copy<T, T>(Uo, U, opts);
    }
    if (wv) {
        // VT := V_B^T VT
        const int64_t b = std::max<int64_t>(1, VT.mb());
        Matrix<T> Vb(n, n, b, b, VT.grid()), Vo(n, VT.n(), b, std::max<int64_t>(1, VT.nb()), VT.grid());
        Vb.insertLocalTiles(target);
        Vo.insertLocalTiles(target);
        internal::bdsdc_place<T>(c, Vb, VB.data(), n, true, no_phase);
        gemm(T(1), Vb, VT, T(0), Vo, opts);
        slate::copy<T, T>(Vo, VT, opts);
    }
}

#define SLATE_BDSDC_INST(T)                                                                               \
    template void bdsdc<T>(Job, Job, std::vector<real_type<T>>&, std::vector<real_type<T>>&, Matrix<T>&, \
                           Matrix<T>&, Options const&);
SLATE_BDSDC_INST(float)
SLATE_BDSDC_INST(double)
SLATE_BDSDC_INST(std::complex<float>)
SLATE_BDSDC_INST(std::complex<double>)

}  // namespace slate
