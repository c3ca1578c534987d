// QR factorization with column pivoting (LAPACK geqp3: laqps panels plus one
// gemm update, written from the math), its back-transform and the rank-aware
// least-squares driver gelsy, real types, on ONE contiguous local array of
// either target.
//
// Each column makes one pass over the trailing matrix, A^T v, which the device
// reads once per column (kernels/geqp3.hip); the pivot search, the swap, the
// norm downdate and the recompute of an untrustworthy norm are device kernels
// too, so jpvt, tau and the counters stay on the device and the only host
// synchronisation is the one that fetches jpvt and the counters at the end.
// LAPACK cuts a panel short when a downdated norm cannot be trusted; here the
// panel goes on: the pending update is applied to that column alone (its row
// of F cleared) and its norm recomputed from the stored entries, so the norm
// and the entries the factorization goes on with are the same bits, as they
// are in LAPACK after its early update.  The trailing update is one lb::gemm per
// panel, the T factors S = V^T V plus the larft recurrence, the back-transform
// one lb::larfb per panel.  The host target runs host::geqp3 (eig_host.cc),
// the same algorithm in plain loops.
#include "reduce_common.hh"

#include <cmath>
#include <limits>

namespace slate {

namespace {
internal::LastStats<Geqp3Stats> g_stats;   // of the last factorization in this process
}  // namespace

Geqp3Stats geqp3_stats() { return g_stats.get(); }

namespace internal {

namespace {
/// SLATE_GEQP3_PROFILE=1 (StageProfile): the kinds of Geqp3Stats::ms_*
enum Geqp3Kind { Pivot = 0, Panel = 1, Product = 2, Gemm = 3, Larft = 4, Kinds = 5 };
}  // namespace

template <typename R>
void geqp3_local(lb::Ctx const& c, int64_t m, int64_t n, R* A, int64_t lda, std::vector<int64_t>& jpvt, R* tau,
                 R* Tfac) {
    namespace kd = slate_amd::dev;
    const int64_t nb = kGeqp3Panel, kmin = std::min(m, n);
    jpvt.assign(n, 0);
    for (int64_t j = 0; j < n; ++j) jpvt[j] = j;
    Geqp3Stats st;
    if (kmin == 0) {
        g_stats.set(st);
        return;
    }
    // T factors: every panel's reflectors are final (later panels touch A(k1:, k1:) only)
    auto t_factors = [&](R* Vx) {
        for (int64_t j0 = 0; j0 < kmin; j0 += nb)
            panel_T_factors<R>(c, m - j0, std::min(nb, kmin - j0), A + j0 + j0 * lda, lda, tau + j0, Tfac + j0 * nb, nb,
                               Vx);
    };
    if (!c.dev()) {
        st.norm_recomputes = host::geqp3<R>(m, n, A, lda, jpvt.data(), tau, nb);
        t_factors(nullptr);
        st.panels = (kmin + nb - 1) / nb;
        st.columns = kmin;
        g_stats.set(st);
        return;
    }
    slate_error_if_msg(n >= (int64_t(1) << 31), "geqp3: more than 2^31 - 1 columns");
    hipStream_t s = c.stream;
    const int64_t ndot = (m + 255) / 256, nrm = (m + 63) / 64;
    Work<R> F(Target::Devices, size_t(n) * nb), vec(Target::Devices, size_t(m) + 2 * n + 1 + nrm + 64 * ndot);
    Work<R> part(Target::Devices, size_t(m / 256 + 2) * n);
    // jpvt | recomputes | piv | flag (int, two to a slot)
    Work<int64_t> ints(Target::Devices, size_t(2 * n + 1 + (n + 1) / 2));
    kd::Geqp3Work<R> wk;
    wk.F = F.data(); wk.ldf = n;
    R* p = vec.data();
    wk.v = p; p += m;
    wk.vn1 = p; p += n;
    wk.vn2 = p; p += n;
    wk.scal = p; p += 1;
    wk.ssq = p; p += nrm;
    wk.pdots = p;
    wk.tau = tau;
    wk.colpart = part.data();
    wk.jpvt = ints.data();
    wk.recomputes = ints.data() + n;
    wk.piv = ints.data() + 2 * n;
    wk.flag = reinterpret_cast<int*>(ints.data() + 2 * n + 1);
    wk.tol3z = std::sqrt(std::numeric_limits<R>::epsilon() / 2);
    StageProfile prof("SLATE_GEQP3_PROFILE", Kinds, s);
    prof.mark(StageProfile::Start);
    kd::geqp3_norms<R>(m, n, A, lda, wk, s);
    ++st.launches_norms;
    prof.mark(Panel);
    for (int64_t j0 = 0; j0 < kmin; j0 += nb) {
        const int64_t kb = std::min(nb, kmin - j0), k1 = j0 + kb;
        {
            trace::Block tp("geqp3_panel");
            for (int64_t j = j0; j < k1; ++j) {
                if (j + 1 < n) {
                    kd::geqp3_pivot<R>(n, j, wk, s);
                    kd::geqp3_swap<R>(m, j, j0, A, lda, wk, s);
                    ++st.launches_pivot;
                    ++st.launches_swap;
                    prof.mark(Pivot);
                }
                kd::geqp3_column<R>(m, j, j0, A, lda, wk, s);
                kd::geqp3_larfg<R>(m, j, A, lda, wk, s);
                ++st.launches_column;
                ++st.launches_larfg;
                prof.mark(Panel);
                if (j + 1 >= n) break;
                kd::geqp3_product<R>(m, n, j, j0, A, lda, wk, s);
                prof.mark(Product);
                kd::geqp3_finish<R>(m, n, j, j0, A, lda, wk, s);
                kd::geqp3_recompute<R>(m, n, j, j0, A, lda, wk, s);
                ++st.launches_product;
                ++st.launches_finish;
                ++st.launches_recompute;
                prof.mark(Panel);
            }
        }
        st.columns += kb;
        ++st.panels;
        if (k1 < n && k1 < m) {
            trace::Block tu("geqp3_gemm");
            lb::gemm(c, Op::NoTrans, Op::Trans, m - k1, n - k1, kb, R(-1), A + k1 + j0 * lda, lda, wk.F + k1, wk.ldf,
                     R(1), A + k1 + k1 * lda, lda);
            prof.mark(Gemm);
        }
    }
    {
        trace::Block tt("geqp3_larft");
        Work<R> Vx(Target::Devices, size_t(m) * nb);
        t_factors(Vx.data());
        prof.mark(Larft);
    }
    // jpvt and the counters, contiguous on the device: one copy
    std::vector<int64_t> both(size_t(2 * n));
    device::memcpy_async(both.data(), ints.data(), size_t(2 * n) * sizeof(int64_t), s);
    slate_hip_call(hipStreamSynchronize(s));
    st.host_syncs = 1;
    std::copy(both.begin(), both.begin() + n, jpvt.begin());
    for (int64_t j = 0; j < n; ++j) st.norm_recomputes += both[n + j];
    const std::vector<double> ms = prof.finish();
    st.ms_pivot = ms[Pivot]; st.ms_panel = ms[Panel]; st.ms_product = ms[Product]; st.ms_gemm = ms[Gemm];
    st.ms_larft = ms[Larft];
    g_stats.set(st);
}

template <typename R>
void unmqr_geqp3_local(lb::Ctx const& c, Side side, Op op, int64_t m, int64_t n, R const* A, int64_t lda,
                       R const* Tfac, int64_t mc, int64_t nc, R* C, int64_t ldc) {
    slate_error_if_msg((side == Side::Left ? mc : nc) != m, "unmqr_geqp3: C does not match Q");
    apply_panel_reflectors<R>(c, side, op, std::min(m, n), 0, [&](int64_t j0, int64_t, int64_t& ldv) {
        ldv = lda;
        return A + j0 + j0 * lda;
    }, Tfac, mc, nc, C, ldc);
}

#define SLATE_GEQP3_LOCAL_INST(R)                                                                                  \
    template void geqp3_local<R>(lb::Ctx const&, int64_t, int64_t, R*, int64_t, std::vector<int64_t>&, R*, R*);    \
    template void unmqr_geqp3_local<R>(lb::Ctx const&, Side, Op, int64_t, int64_t, R const*, int64_t, R const*,    \
                                       int64_t, int64_t, R*, int64_t);
SLATE_GEQP3_LOCAL_INST(float)
SLATE_GEQP3_LOCAL_INST(double)

}  // namespace internal

//------------------------------------------------------------------------------
template <typename T>
void geqp3(Matrix<T>& A, std::vector<int64_t>& jpvt, TriangularFactors<T>& T_, Options const& opts) {
    trace::Block tb("geqp3");
    internal::DriverScope ds_;
    internal::geqp3_check_operand<T>(A, "geqp3", "A");
    if constexpr (!is_complex_v<T>) {
        slate_error_if_msg(A.op() != Op::NoTrans || !A.aligned(), "geqp3: a whole NoTrans matrix is required");
        const Target target = internal::resolve_target(opts);
        const int64_t m = A.m(), n = A.n(), nb = internal::kGeqp3Panel;
        T_ = internal::make_panel_factors<T>(n, nb, target, opts);
        if (m == 0 || n == 0) {
            // nothing to factor and no launch: jpvt = identity, the counters cleared
            internal::geqp3_local<T>(lb::Ctx::host(), m, n, nullptr, 1, jpvt, nullptr, nullptr);
            return;
        }
        const Loc loc = internal::loc_of(target);
        LocalBlock<T> la = A.local(loc, true);
        LocalBlock<T> lt = T_[0].local(loc, true), ltau = T_[1].local(loc, true);
        slate_error_if_msg(la.m != m || la.n != n || lt.ld != nb, "geqp3: unexpected local layout");
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        internal::geqp3_local<T>(c, m, n, la.ptr, la.ld, jpvt, ltau.ptr, lt.ptr);
        internal::finish_origin(A, opts);
    }
}

template <typename T>
void unmqr_geqp3(Side side, Op op, Matrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& C, Options const& opts) {
    trace::Block tb("unmqr_geqp3");
    internal::DriverScope ds_;
    internal::geqp3_check_operand<T>(A, "unmqr_geqp3", "A");
    internal::geqp3_check_operand<T>(C, "unmqr_geqp3", "C");
    if constexpr (!is_complex_v<T>) {
        const int64_t m = A.m(), n = A.n(), nb = internal::kGeqp3Panel;
        slate_error_if_msg(A.op() != Op::NoTrans || !A.aligned(), "unmqr_geqp3: A as geqp3 left it");
        slate_error_if_msg(T_.empty() || T_[0].m() != nb || T_[0].n() < n, "unmqr_geqp3: T is not from geqp3");
        slate_error_if_msg(C.op() != Op::NoTrans || !C.aligned(), "unmqr_geqp3: a whole NoTrans C is required");
        if (m == 0 || n == 0 || C.m() == 0 || C.n() == 0) return;
        const Target target = internal::resolve_target(opts);
        const Loc loc = internal::loc_of(target);
        LocalBlock<T> la = A.local(loc, false), lt = T_[0].local(loc, false), lc = C.local(loc, true);
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        internal::unmqr_geqp3_local<T>(c, side, op, m, n, la.ptr, la.ld, lt.ptr, C.m(), C.n(), lc.ptr, lc.ld);
        if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
        internal::finish_origin(C, opts);
    }
}

template <typename T>
int64_t gelsy(Matrix<T>& A, Matrix<T>& BX, real_type<T> rcond, Options const& opts) {
    trace::Block tb("gelsy");
    internal::DriverScope ds_;
    internal::geqp3_check_operand<T>(A, "gelsy", "A");
    internal::geqp3_check_operand<T>(BX, "gelsy", "BX");
    int64_t rank = 0;
    if constexpr (!is_complex_v<T>) {
        namespace kd = slate_amd::dev;
        const int64_t m = A.m(), n = A.n(), nrhs = BX.n(), kmin = std::min(m, n);
        slate_error_if_msg(A.op() != Op::NoTrans || !A.aligned() || BX.op() != Op::NoTrans || !BX.aligned(),
                           "gelsy: whole NoTrans matrices are required");
        slate_error_if_msg(BX.m() != std::max(m, n), "gelsy: BX is max(m, n) x nrhs");
        if (n == 0 || nrhs == 0) return 0;
        const Target target = internal::resolve_target(opts);
        const Loc loc = internal::loc_of(target);
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        // 1: the range guard of svd
        T anorm = T(0), alpha = T(1);
        if (kmin > 0) {
            anorm = slate::norm(Norm::Max, A, opts);
            bool bad = false;
            alpha = internal::range_alpha(anorm, bad);
            if (bad) {
                LocalBlock<T> lx = BX.local(loc, true);
                lb::set(c, Uplo::General, n, nrhs, std::numeric_limits<T>::quiet_NaN(),
                        std::numeric_limits<T>::quiet_NaN(), lx.ptr, lx.ld);
                if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
                internal::finish_origin(BX, opts);
                return 0;
            }
            if (alpha != T(1)) scale(alpha, anorm, A, opts);
        }
        // 2: A P = Q R
        std::vector<int64_t> jpvt;
        TriangularFactors<T> Tf;
        geqp3(A, jpvt, Tf, opts);
        LocalBlock<T> lx = BX.local(loc, true);
        // 3: the rank by the plain diagonal rule
        if (kmin > 0) {
            LocalBlock<T> la = A.local(loc, false);
            std::vector<T> dg(kmin);
            if (c.dev()) {
                device::memcpy2d_async(dg.data(), sizeof(T), la.ptr, size_t(la.ld + 1) * sizeof(T), sizeof(T),
                                       size_t(kmin), c.stream);
                slate_hip_call(hipStreamSynchronize(c.stream));
            } else {
                for (int64_t k = 0; k < kmin; ++k) dg[k] = la.ptr[k + k * la.ld];
            }
            while (rank < kmin && std::abs(dg[rank]) > rcond * std::abs(dg[0])) ++rank;
        }
        if (rank == 0) {
            lb::set(c, Uplo::General, n, nrhs, T(0), T(0), lx.ptr, lx.ld);
        } else {
            LocalBlock<T> la = A.local(loc, false), lt = Tf[0].local(loc, false);
            // 4: C = (Q^T B)(0:rank)
            internal::unmqr_geqp3_local<T>(c, Side::Left, Op::Trans, m, n, la.ptr, la.ld, lt.ptr, m, nrhs, lx.ptr, lx.ld);
            // 5: the minimum-norm solution y of [R11 R12] y = C, n x nrhs at yp
            internal::Work<T> ybuf;
            Matrix<T> Y;
            T const* yp = nullptr;
            int64_t ldy = 0;
            if (rank == n) {
                lb::trsm(c, Side::Left, Uplo::Upper, Op::NoTrans, Diag::NonUnit, n, nrhs, T(1), la.ptr, la.ld, lx.ptr,
                         lx.ld);
                ybuf.resize(target, size_t(n) * nrhs);
                lb::copy2d(c, n, nrhs, lx.ptr, lx.ld, ybuf.data(), n);
                yp = ybuf.data();
                ldy = n;
            } else {
                // the rank x n row block [R11 R12] on its own, zero below the diagonal, through gels' LQ path
                const int64_t nbw = A.nb();
                Matrix<T> W(rank, n, nbw, nbw, Grid::self());
                Y = Matrix<T>(n, nrhs, nbw, nbw, Grid::self());
                W.insertLocalTiles(target);
                Y.insertLocalTiles(target);
                LocalBlock<T> lw = W.local(loc, true), ly = Y.local(loc, true);
                lb::copy2d(c, rank, n, la.ptr, la.ld, lw.ptr, lw.ld);
                if (rank > 1) lb::set(c, Uplo::Lower, rank - 1, rank - 1, T(0), T(0), lw.ptr + 1, lw.ld);
                lb::set(c, Uplo::General, n, nrhs, T(0), T(0), ly.ptr, ly.ld);
                lb::copy2d(c, rank, nrhs, lx.ptr, lx.ld, ly.ptr, ly.ld);
                if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
                TriangularFactors<T> Tw;
                gels(W, Tw, Y, opts);
                LocalBlock<T> ly2 = Y.local(loc, false);
                yp = ly2.ptr;
                ldy = ly2.ld;
                lx = BX.local(loc, true);
            }
            // 6: X = P y
            if (c.dev()) {
                internal::Work<int64_t> jd(Target::Devices, size_t(n));
                device::memcpy_async(jd.data(), jpvt.data(), size_t(n) * sizeof(int64_t), c.stream);
                kd::geqp3_scatter_rows<T>(n, nrhs, jd.data(), yp, ldy, lx.ptr, lx.ld, c.stream);
                slate_hip_call(hipStreamSynchronize(c.stream));
            } else {
                for (int64_t k = 0; k < nrhs; ++k)
                    for (int64_t i = 0; i < n; ++i) lx.ptr[jpvt[i] + k * lx.ld] = yp[i + k * ldy];
            }
            // A was scaled by alpha / anorm, so the solution of the scaled problem is X anorm / alpha
            if (alpha != T(1)) lb::scale(c, Uplo::General, n, nrhs, alpha, anorm, lx.ptr, lx.ld);
        }
        if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
        internal::finish_origin(BX, opts);
    }
    return rank;
}

#define SLATE_GEQP3_INST(T)                                                                                        \
    template void geqp3<T>(Matrix<T>&, std::vector<int64_t>&, TriangularFactors<T>&, Options const&);              \
    template void unmqr_geqp3<T>(Side, Op, Matrix<T>&, TriangularFactors<T>&, Matrix<T>&, Options const&);         \
    template int64_t gelsy<T>(Matrix<T>&, Matrix<T>&, real_type<T>, Options const&);
SLATE_GEQP3_INST(float)
SLATE_GEQP3_INST(double)
SLATE_GEQP3_INST(std::complex<float>)
SLATE_GEQP3_INST(std::complex<double>)

}  // namespace slate
