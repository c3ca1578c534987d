// Distributed stage 2 of the eigensolver: tridiagonal divide and conquer with
// the eigenvector matrix on the 2-D process grid (reference src/stedc.cc,
// stedc_solve.cc, stedc_merge.cc:171-190, stedc_z_vector.cc, stedc_sort.cc,
// stedc_deflate.cc, stedc_secular.cc) and the QR iteration with distributed
// eigenvector rows (reference src/steqr2.cc:60-74, {s,d,c,z}steqr2.f).
//
// stedc_dist.  The tridiagonal (d, e) is replicated (O(n)); Q lives ONLY in
// the distributed matrix (device instance on the device target).  The split
// tree follows Q's tiles: every leaf is one diagonal tile, solved by its owner
// on the host (nb x nb); every merge of two adjacent tile ranges
// [lo, mid) + [mid, hi):
//   * z = rows mid-1 / mid of Q over the block's columns: one world all-reduce
//     of n2 values;
//   * sort, deflation (tiny z, close pairs -> Givens rotations recorded, not
//     applied) on the host, replicated and deterministic: O(n2 log n2);
//   * secular roots (one wave per root) and Gu-Eisenstat z on the device;
//   * the merge matrix M (Q_new = Q_old M, n2 x n2) built by every rank for
//     its OWN local entries only -- both through dc_merge.hh, the merge
//     shared with bdsdc (kernels/dc_merge.hip, host twins in dc_merge.cc);
//   * Q_new = [Q1 0; 0 Q2] M as two distributed MFMA GEMMs on the halves.
// No rank holds an n x n array on the host: per-rank host memory is O(n + nb^2).
//
// steqr2_dist.  Implicit QL (the host steqr's sweeps) on the replicated
// (d, e); every plane rotation acts on two columns of Z, i.e. row-wise, so
// with Z laid out by rows (P x 1 grid) each rank applies the rotations to its
// own rows with no communication -- on the device through the batched
// wavefront rotation kernel of bdsqr.
#include "internal.hh"
#include "dc_merge.hh"
#include "eig_sinks.hh"
#include "slate_amd/eig_host.hh"
#include "../kernels/kernels.hh"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace slate {
namespace internal {

namespace {

struct SplitNode { int64_t t0, tm, t1; double beta; };

/// post-order merge list of the tile-aligned bisection tree over tiles [t0, t1)
void split_tree(int64_t t0, int64_t t1, std::vector<SplitNode>& merges, std::vector<int64_t>& cuts) {
    if (t1 - t0 <= 1) return;
    const int64_t tm = (t0 + t1) / 2;
    split_tree(t0, tm, merges, cuts);
    split_tree(tm, t1, merges, cuts);
    merges.push_back({t0, tm, t1, 0.0});
    cuts.push_back(tm);
}

}  // namespace

template <typename R>
void stedc_dist(std::vector<R>& d, std::vector<R> const& e_in, Matrix<R>& Q, Options const& opts) {
    trace::Block tb("stedc_dist");
    internal::DriverScope ds_;
    const Target target = resolve_target(opts);
    const Loc loc = loc_of(target);
    const int64_t n = int64_t(d.size());
    slate_error_if_msg(Q.m() != n || Q.n() != n || Q.mb() != Q.nb() || !Q.aligned() || Q.op() != Op::NoTrans,
                       "stedc: Q must be an n x n NoTrans matrix with square tiles");
    if (n == 0) return;
    auto& g = *Q.grid();
    Comm& world = g.world();
    lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
    std::vector<R> e(e_in.begin(), e_in.end());
    e.resize(std::max<int64_t>(n - 1, 0));
    const int64_t nt = Q.nt();
    std::vector<SplitNode> merges;
    std::vector<int64_t> cuts;
    split_tree(0, nt, merges, cuts);
    // tear at every cut (Cuppen): T = diag(T1, T2) + |beta| v v^T
    for (auto& nd : merges) {
        const int64_t mid = grow_of(Q, nd.tm);
        nd.beta = double(e[mid - 1]);
        const R rho0 = std::abs(e[mid - 1]);
        d[mid - 1] -= rho0;
        d[mid] -= rho0;
    }
    // ---- leaves: diagonal tiles, solved by their owners
    set(R(0), R(0), Q, opts);
    std::vector<R> dl(n, R(0));
    {
        trace::Block t2("stedc_leaves");
        Q.storage()->get(loc, true);
        for (int64_t t = 0; t < nt; ++t) {
            if (!Q.tileIsLocal(t, t)) continue;
            const int64_t r0 = grow_of(Q, t), nbt = Q.tileNb(t);
            std::vector<R> dt(d.begin() + r0, d.begin() + r0 + nbt), et(std::max<int64_t>(nbt - 1, 0));
            for (int64_t i = 0; i + 1 < nbt; ++i) et[i] = e[r0 + i];
            std::vector<R> Zt(size_t(nbt) * nbt);
            host::stedc<R>(nbt, dt.data(), et.data(), Zt.data(), nbt);
            Tile<R> tl = Q.tile(t, t, loc);
            if (c.dev()) {
                device::memcpy2d_async(tl.data, tl.stride * sizeof(R), Zt.data(), nbt * sizeof(R), nbt * sizeof(R), nbt,
                                       c.stream);
                slate_hip_call(hipStreamSynchronize(c.stream));
            } else {
                for (int64_t j = 0; j < nbt; ++j) std::copy(Zt.begin() + j * nbt, Zt.begin() + (j + 1) * nbt, tl.data + j * tl.stride);
            }
            std::copy(dt.begin(), dt.end(), dl.begin() + r0);
        }
        allreduce_host(world, dl.data(), size_t(n), ReduceOp::Sum);
        d = dl;
    }
    if (merges.empty()) return;
    Matrix<R> Qb = Q.emptyLike(), M = Q.emptyLike();
    Qb.insertLocalTiles(target);
    M.insertLocalTiles(target);
    auto& st = *Q.storage();
    DcMergeWork ws;
    for (auto const& nd : merges) {
        trace::Block t2("stedc_merge");
        const int64_t lo = grow_of(Q, nd.t0), mid = grow_of(Q, nd.tm), hi = grow_of(Q, nd.t1);
        const int64_t n1 = mid - lo, n2 = hi - lo;
        const double rho = 2.0 * std::abs(nd.beta), sgn = nd.beta < 0 ? -1.0 : 1.0;
        // ---- z: row mid-1 of Q over [lo, mid) and row mid over [mid, hi)
        std::vector<double> z(n2, 0.0);
        {
            trace::Block t3("stedc_m_z");
            LocalBlock<R> lq = Q.local(loc, false);
            auto grab = [&](int64_t grow, int64_t c0, int64_t c1, double scl) {
                if (st.row_owner(grow / st.mb) != g.myrow()) return;
                const int64_t lr = g2l(grow, st.mb, g.p());
                const int64_t lc0 = g2l_ceil(c0, st.nb, st.crel(), g.q()), lc1 = g2l_ceil(c1, st.nb, st.crel(), g.q());
                if (lc1 <= lc0) return;
                std::vector<R> row(lc1 - lc0);
                if (c.dev()) {
                    device::memcpy2d_async(row.data(), sizeof(R), lq.ptr + lr + lc0 * lq.ld, lq.ld * sizeof(R),
                                           sizeof(R), lc1 - lc0, c.stream);
                    slate_hip_call(hipStreamSynchronize(c.stream));
                } else {
                    for (int64_t t = lc0; t < lc1; ++t) row[t - lc0] = lq.ptr[lr + t * lq.ld];
                }
                for (int64_t t = lc0; t < lc1; ++t)
                    z[l2g(t, st.nb, st.crel(), g.q()) - lo] = scl * double(row[t - lc0]);
            };
            const double s2 = 1.0 / std::sqrt(2.0);
            grab(mid - 1, lo, mid, s2);
            grab(mid, mid, hi, sgn * s2);
            allreduce_host(world, z.data(), size_t(n2), ReduceOp::Sum);
        }
        // ---- sort (stable), deflation (rotations recorded)
        std::vector<int64_t> perm(n2);
        std::iota(perm.begin(), perm.end(), int64_t(0));
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return d[lo + a] < d[lo + b]; });
        std::vector<double> Ds(n2), zs(n2);
        for (int64_t s = 0; s < n2; ++s) { Ds[s] = double(d[lo + perm[s]]); zs[s] = z[perm[s]]; }
        std::vector<char> defl_flag(n2, 0);
        RotationList rot;
        {
            trace::Block t3("stedc_m_deflate");
            const double eps = std::numeric_limits<R>::epsilon();
            double dmax = 0, zmax = 0;
            for (int64_t j = 0; j < n2; ++j) { dmax = std::max(dmax, std::abs(Ds[j])); zmax = std::max(zmax, std::abs(zs[j])); }
            const double tol = 8.0 * eps * std::max(dmax, zmax * rho);
            for (int64_t j = 0; j < n2; ++j) defl_flag[j] = (rho * std::abs(zs[j]) <= tol) ? 1 : 0;
            int64_t last = -1;
            for (int64_t j = 0; j < n2; ++j) {
                if (defl_flag[j]) continue;
                if (last >= 0 && close_pole_rotation(Ds, zs, last, j, tol, {&rot})) defl_flag[last] = 1;
                last = j;
            }
        }
        std::vector<int64_t> act, defl;
        for (int64_t j = 0; j < n2; ++j) (defl_flag[j] ? defl : act).push_back(j);
        std::sort(act.begin(), act.end(), [&](int64_t a, int64_t b) { return Ds[a] < Ds[b]; });
        const int64_t k = int64_t(act.size());
        std::vector<double> dd(k), zz(k);
        for (int64_t i = 0; i < k; ++i) { dd[i] = Ds[act[i]]; zz[i] = zs[act[i]]; }
        // a loop of its own: fused with the gather above, g++ fuses the products into the sum and the last
        // root, with it the results pinned by test_stedc_bitwise_unchanged, move by an ulp
        double znorm2 = 0;
        for (int64_t i = 0; i < k; ++i) znorm2 += zz[i] * zz[i];
        // ---- secular roots (device or host), eigenvalues, output order
        std::vector<int64_t> org;
        std::vector<double> tau, zh;
        trace::Block t3s("stedc_m_secular");
        secular_solve<secular::LinearPoles<double>>(c, ws, n2, rot.count(), k, rho, dd, zz, znorm2, org, tau, zh);
        t3s.end();
        std::vector<double> lam(n2);
        for (int64_t r = 0; r < k; ++r) lam[r] = dd[org[r]] + tau[r];
        for (int64_t cdx = 0; cdx < n2 - k; ++cdx) lam[k + cdx] = Ds[defl[cdx]];
        std::vector<int64_t> ord(n2), inv_perm(n2);
        std::iota(ord.begin(), ord.end(), int64_t(0));
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return lam[a] < lam[b]; });
        for (int64_t s = 0; s < n2; ++s) inv_perm[perm[s]] = s;
        // ---- merge matrix: my local entries of the n2 x n2 block
        trace::Block t3m("stedc_m_matrix");
        Matrix<R> Mb = M.sub(nd.t0, nd.t1 - 1, nd.t0, nd.t1 - 1);
        LocalBlock<R> lm = Mb.local(loc, true);
        StedcSide side;
        side.lrows = lm.m; side.mb = st.mb; side.p = g.p(); side.rrel = st.rrel(); side.row_off = lo;
        side.nb = st.nb; side.q = g.q(); side.crel = st.crel(); side.col_off = lo;
        side.lr0 = Mb.lrow_begin(); side.lc0 = Mb.lcol_begin();
        DcRotations drot;
        const DcMerge mg = merge_layout(c, ws, n2, dd, zh, tau, org, act, defl, ord, inv_perm, {&rot}, &drot);
        merge_columns<R>(c, ws, mg, drot, side, lm.n, lm.ptr, lm.ld);
        if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
        t3m.end();
        // ---- Q_new = [Q1 0; 0 Q2] M  (two GEMMs on the halves), back into Q
        {
            trace::Block t3("stedc_m_gemm");
            Matrix<R> Q1 = Q.sub(nd.t0, nd.tm - 1, nd.t0, nd.tm - 1), Q2 = Q.sub(nd.tm, nd.t1 - 1, nd.tm, nd.t1 - 1);
            Matrix<R> Mt = M.sub(nd.t0, nd.tm - 1, nd.t0, nd.t1 - 1), Mbot = M.sub(nd.tm, nd.t1 - 1, nd.t0, nd.t1 - 1);
            Matrix<R> Ct = Qb.sub(nd.t0, nd.tm - 1, nd.t0, nd.t1 - 1), Cb = Qb.sub(nd.tm, nd.t1 - 1, nd.t0, nd.t1 - 1);
            gemm(R(1), Q1, Mt, R(0), Ct, opts);
            gemm(R(1), Q2, Mbot, R(0), Cb, opts);
            Matrix<R> Qd = Q.sub(nd.t0, nd.t1 - 1, nd.t0, nd.t1 - 1), Qs = Qb.sub(nd.t0, nd.t1 - 1, nd.t0, nd.t1 - 1);
            slate::copy<R, R>(Qs, Qd, opts);
        }
        for (int64_t jo = 0; jo < n2; ++jo) d[lo + jo] = R(lam[ord[jo]]);
        (void)n1;
    }
}

//------------------------------------------------------------------------------
namespace {

/// Rotations of the QL sweeps applied to the local rows of Z (rows are
/// independent under column rotations).  QL sweeps run with i descending; on
/// the column-reversed Z (column j' = n-1-j: base Z + (n-1) ld, leading
/// dimension -ld) they are ASCENDING sweeps of the rotations (n-2-i, c, -s),
/// which the bdsqr row sink batches into its wavefront tables -- the device
/// kernel and its host twin alike, so the CPU tests check the reflection.
template <typename T>
struct QlRowSink : host::RotSink<real_type<T>> {
    using R = real_type<T>;
    lb::Ctx c;
    int64_t n, rows, ld;
    T* Z;
    RowRotSink<T> rs;
    std::vector<host::PlaneRot<R>> none;
    QlRowSink(lb::Ctx const& c_, int64_t n_, T* Z_, int64_t ld_, int64_t rows_)
        : c(c_), n(n_), rows(rows_), ld(ld_), Z(Z_), rs(c_, n_) {
        rs.U = rows > 0 ? Z + (n - 1) * ld : nullptr;
        rs.ldu = -ld;
        rs.urows = rows;
    }
    void flush() { rs.finish(); }
    void sweep(std::vector<host::PlaneRot<R>>& ru, std::vector<host::PlaneRot<R>>&) override {
        std::vector<host::PlaneRot<R>> asc(ru.size());
        for (size_t t = 0; t < ru.size(); ++t) asc[t] = {n - 2 - ru[t].i, ru[t].c, -ru[t].s};
        std::sort(asc.begin(), asc.end(), [](auto const& a, auto const& b) { return a.i < b.i; });
        none.clear();
        rs.sweep(asc, none);
    }
    void rot_u(int64_t, int64_t, R, R) override { slate_error("steqr2: unexpected rotation"); }
    void negate_v(int64_t) override {}
    void permute(std::vector<int64_t> const& perm) override {
        flush();
        if (rows <= 0) return;
        Work<T> tmp(c.dev() ? Target::Devices : Target::HostTask, size_t(rows) * n);
        if (c.dev()) {
            Work<int64_t> dp(Target::Devices, perm.size());
            device::memcpy_async(dp.data(), perm.data(), perm.size() * sizeof(int64_t), c.stream);
            slate_amd::dev::rbt_gather(false, false, n, rows, dp.data(), slate_amd::dev::dptr(Z), ld,
                                       slate_amd::dev::dptr(tmp.data()), rows, c.stream);
            lb::copy2d(c, rows, n, tmp.data(), rows, Z, ld);
            slate_hip_call(hipStreamSynchronize(c.stream));
            return;
        }
        for (int64_t i = 0; i < n; ++i)
            for (int64_t r = 0; r < rows; ++r) tmp.data()[r + i * rows] = Z[r + perm[i] * ld];
        for (int64_t i = 0; i < n; ++i)
            for (int64_t r = 0; r < rows; ++r) Z[r + i * ld] = tmp.data()[r + i * rows];
    }
};

}  // namespace

template <typename T>
int64_t steqr2_dist(std::vector<real_type<T>>& d, std::vector<real_type<T>>& e_in, Matrix<T>& Z, Options const& opts) {
    trace::Block tb("steqr2_dist");
    internal::DriverScope ds_;
    using R = real_type<T>;
    const Target target = resolve_target(opts);
    const Loc loc = loc_of(target);
    const int64_t n = int64_t(d.size());
    if (n == 0) return 0;
    std::vector<R> e(e_in.begin(), e_in.end());
    e.resize(std::max<int64_t>(n - 1, 0));
    // Z by rows (P x 1 grid): every rank owns whole rows
    auto g = Z.grid();
    GridPtr gr = col_grid(g);
    const bool rowlayout = (g->q() == 1 && Z.op() == Op::NoTrans && Z.aligned());
    Matrix<T> Zr = rowlayout ? Z : Matrix<T>(Z.m(), Z.n(), Z.mb(), std::max<int64_t>(Z.n(), 1), gr);
    if (!rowlayout) {
        Zr.insertLocalTiles(target);
        slate::copy<T, T>(Z, Zr, opts);
    }
    LocalBlock<T> lz = Zr.local(loc, true);
    lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
    QlRowSink<T> sink(c, n, lz.ptr, lz.ld, lz.m);
    int64_t info = host::steqr_core<R>(n, d.data(), e.data(), &sink);
    sink.flush();
    if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
    if (!rowlayout) slate::copy<T, T>(Zr, Z, opts);
    else internal::finish_origin(Z, opts);
    return info;
}

template void stedc_dist<float>(std::vector<float>&, std::vector<float> const&, Matrix<float>&, Options const&);
template void stedc_dist<double>(std::vector<double>&, std::vector<double> const&, Matrix<double>&, Options const&);
template int64_t steqr2_dist<float>(std::vector<float>&, std::vector<float>&, Matrix<float>&, Options const&);
template int64_t steqr2_dist<double>(std::vector<double>&, std::vector<double>&, Matrix<double>&, Options const&);
template int64_t steqr2_dist<std::complex<float>>(std::vector<float>&, std::vector<float>&,
                                                  Matrix<std::complex<float>>&, Options const&);
template int64_t steqr2_dist<std::complex<double>>(std::vector<double>&, std::vector<double>&,
                                                   Matrix<std::complex<double>>&, Options const&);

}  // namespace internal
}  // namespace slate
