// One-stage tridiagonal reduction (LAPACK sytrd: latrd panels plus syr2k
// updates, written from the math) and its back-transform, real types, lower
// triangle, on ONE contiguous local array of either target.
//
// Half of the flops are one symmetric matrix-vector product per column: on
// the device it reads the stored triangle once per product (kernels/hetrd.hip),
// the panel steps are multi-workgroup kernels whose reductions are two-level
// and deterministic, and d, e, tau stay on the device: the only host
// synchronisation is the one that fetches d and e at the end.  The trailing
// updates are lb::syr2k, the T factors S = V^T V plus the larft recurrence, the
// back-transform one lb::larfb per panel.  The host target runs host::hetrd
// (eig_host.cc), the same algorithm in plain loops.
#include "reduce_common.hh"

namespace slate {

namespace {
internal::LastStats<HetrdStats> g_stats;   // of the last reduction in this process
}  // namespace

HetrdStats hetrd_stats() { return g_stats.get(); }

namespace lb {

template <typename R>
void symv_lower(Ctx const& c, int64_t m, R const* A, int64_t lda, R const* x, R* y) {
    if (m <= 0) return;
    if (!c.dev()) {
        for (int64_t i = 0; i < m; ++i) y[i] = A[i + i * lda] * x[i];
        for (int64_t j = 0; j < m; ++j)
            for (int64_t i = j + 1; i < m; ++i) {
                y[i] += A[i + j * lda] * x[j];
                y[j] += A[i + j * lda] * x[i];
            }
        return;
    }
    Scratch sc(c);
    R* work = sc.alloc<R>(size_t(slate_amd::dev::symv_lower_workspace(m)));
    slate_amd::dev::symv_lower<R>(m, A, lda, x, y, work, c.stream);
}
template void symv_lower<float>(Ctx const&, int64_t, float const*, int64_t, float const*, float*);
template void symv_lower<double>(Ctx const&, int64_t, double const*, int64_t, double const*, double*);

}  // namespace lb

namespace internal {

namespace {
/// SLATE_HETRD_PROFILE=1 (StageProfile): the kinds of HetrdStats::ms_*
enum HetrdKind { Panel = 0, Symv = 1, Syr2k = 2, Larft = 3, Kinds = 4 };
}  // namespace

template <typename R>
void hetrd_local(lb::Ctx const& c, int64_t n, R* A, int64_t lda, std::vector<R>& d, std::vector<R>& e, R* tau,
                 R* Tfac) {
    namespace kd = slate_amd::dev;
    const int64_t nb = kHetrdPanel;
    d.assign(n, R(0));
    e.assign(std::max<int64_t>(n - 1, 0), R(0));
    if (n == 0) return;
    HetrdStats st;
    // T factors: every panel's V is final (later panels touch A(k1:, k1:) only)
    auto t_factors = [&](R* Vx) {
        for (int64_t j0 = 0; j0 < n - 1; j0 += nb)
            panel_T_factors<R>(c, n - j0 - 1, std::min(nb, n - 1 - j0), A + (j0 + 1) + j0 * lda, lda, tau + j0,
                               Tfac + j0 * nb, nb, Vx);
    };
    if (!c.dev()) {
        std::vector<R> eh(n, R(0));
        host::hetrd<R>(n, A, lda, d.data(), eh.data(), tau, nb);
        std::copy(eh.begin(), eh.begin() + (n - 1), e.begin());
        t_factors(nullptr);
        st.panels = (n - 1 + nb - 1) / nb;
        st.columns = n - 1;
        g_stats.set(st);
        return;
    }
    hipStream_t s = c.stream;
    const int64_t nblk = (n + 255) / 256, nrblk = (n + 63) / 64;   // workgroups of the dots, of the row kernels
    Work<R> W(Target::Devices, size_t(n) * nb), vec(Target::Devices, size_t(4) * n + 1 + 2 * nrblk + 128 * nblk);
    Work<R> part(Target::Devices, size_t(n / 16 + 2) * n + size_t(n / 64 + 2) * n);
    kd::HetrdWork<R> wk;
    wk.W = W.data(); wk.ldw = n;
    R* p = vec.data();
    wk.v = p; p += n;
    wk.wraw = p; p += n;
    wk.d = p; p += n;
    wk.e = p; p += n;
    wk.scal = p; p += 1;
    wk.ssq = p; p += nrblk;
    wk.pdot = p; p += nrblk;
    wk.pvw = p;
    wk.tau = tau;
    wk.rowpart = part.data();
    wk.colpart = part.data() + size_t(n / 16 + 2) * n;
    StageProfile prof("SLATE_HETRD_PROFILE", Kinds, s);
    prof.mark(StageProfile::Start);
    for (int64_t j0 = 0; j0 < n - 1; j0 += nb) {
        const int64_t kb = std::min(nb, n - 1 - j0), k1 = j0 + kb;
        {
            trace::Block tp("hetrd_panel");
            for (int64_t i = j0; i < k1; ++i) {
                kd::hetrd_column<R>(n, i, j0, true, A, lda, wk, s);
                kd::hetrd_larfg<R>(n, i, A, lda, wk, s);
                prof.mark(Panel);
                kd::hetrd_symv<R>(n, i, j0, A, lda, wk, s);
                prof.mark(Symv);
                kd::hetrd_correct<R>(n, i, j0, A, lda, wk, s);
            }
            kd::hetrd_column<R>(n, k1, j0, false, A, lda, wk, s);   // last column of W
            prof.mark(Panel);
        }
        st.launches_column += kb + 1;
        st.launches_larfg += kb;
        st.launches_symv += kb;
        st.launches_correct += kb;
        st.columns += kb;
        ++st.panels;
        trace::Block tu("hetrd_syr2k");
        lb::syr2k(c, Uplo::Lower, Op::NoTrans, n - k1, kb, R(-1), A + k1 + j0 * lda, lda, wk.W + k1, wk.ldw, R(1),
                  A + k1 + k1 * lda, lda);
        prof.mark(Syr2k);
    }
    device::memcpy_async(wk.d + (n - 1), A + (n - 1) + (n - 1) * lda, sizeof(R), s);
    {
        trace::Block tt("hetrd_larft");
        Work<R> Vx(Target::Devices, size_t(n) * nb);
        t_factors(Vx.data());
        prof.mark(Larft);
    }
    device::memcpy_async(d.data(), wk.d, size_t(n) * sizeof(R), s);
    if (n > 1) device::memcpy_async(e.data(), wk.e, size_t(n - 1) * sizeof(R), s);
    slate_hip_call(hipStreamSynchronize(s));
    st.host_syncs = 1;
    const std::vector<double> ms = prof.finish();
    st.ms_panel = ms[Panel]; st.ms_symv = ms[Symv]; st.ms_syr2k = ms[Syr2k]; st.ms_larft = ms[Larft];
    g_stats.set(st);
}

template <typename R>
void unmtr_hetrd_local(lb::Ctx const& c, Side side, Op op, int64_t n, R const* A, int64_t lda, R const* Tfac,
                       int64_t mc, int64_t nc, R* C, int64_t ldc) {
    slate_error_if_msg((side == Side::Left ? mc : nc) != n, "unmtr_hetrd: C does not match Q");
    apply_panel_reflectors<R>(c, side, op, n - 1, 1, [&](int64_t j0, int64_t, int64_t& ldv) {
        ldv = lda;
        return A + (j0 + 1) + j0 * lda;
    }, Tfac, mc, nc, C, ldc);
}

#define SLATE_HETRD_LOCAL_INST(R)                                                                              \
    template void hetrd_local<R>(lb::Ctx const&, int64_t, R*, int64_t, std::vector<R>&, std::vector<R>&, R*, R*); \
    template void unmtr_hetrd_local<R>(lb::Ctx const&, Side, Op, int64_t, R const*, int64_t, R const*, int64_t, \
                                       int64_t, R*, int64_t);
SLATE_HETRD_LOCAL_INST(float)
SLATE_HETRD_LOCAL_INST(double)

}  // namespace internal

//------------------------------------------------------------------------------
template <typename T>
void hetrd(HermitianMatrix<T>& A, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E,
           TriangularFactors<T>& T_, Options const& opts) {
    trace::Block tb("hetrd");
    internal::DriverScope ds_;
    internal::hetrd_check_operand<T>(A, "hetrd", "A");
    if constexpr (!is_complex_v<T>) {
        slate_error_if_msg(A.uplo() != Uplo::Lower || A.op() != Op::NoTrans,
                           "hetrd: the lower triangle of a NoTrans matrix is reduced (Uplo::Upper is not supported)");
        const Target target = internal::resolve_target(opts);
        const int64_t n = A.n(), nb = internal::kHetrdPanel;
        Matrix<T> Ag(A);
        Ag.set_uplo(Uplo::General);
        slate_error_if_msg(!Ag.aligned(), "hetrd: a whole matrix is required");
        T_ = internal::make_panel_factors<T>(n, nb, target, opts);
        D.assign(n, T(0));
        E.assign(std::max<int64_t>(n - 1, 0), T(0));
        if (n == 0) return;
        const Loc loc = internal::loc_of(target);
        LocalBlock<T> la = Ag.local(loc, true), lt = T_[0].local(loc, true), ltau = T_[1].local(loc, true);
        slate_error_if_msg(la.m != n || la.n != n || lt.ld != nb, "hetrd: unexpected local layout");
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        internal::hetrd_local<T>(c, n, la.ptr, la.ld, D, E, ltau.ptr, lt.ptr);
        internal::finish_origin(Ag, opts);
    }
}

template <typename T>
void unmtr_hetrd(Side side, Op op, HermitianMatrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& C,
                 Options const& opts) {
    trace::Block tb("unmtr_hetrd");
    internal::DriverScope ds_;
    internal::hetrd_check_operand<T>(A, "unmtr_hetrd", "A");
    internal::hetrd_check_operand<T>(C, "unmtr_hetrd", "C");
    if constexpr (!is_complex_v<T>) {
        const int64_t n = A.n(), nb = internal::kHetrdPanel;
        slate_error_if_msg(A.uplo() != Uplo::Lower || A.op() != Op::NoTrans, "unmtr_hetrd: A as hetrd left it");
        slate_error_if_msg(T_.empty() || T_[0].m() != nb || T_[0].n() < n, "unmtr_hetrd: T is not from hetrd");
        slate_error_if_msg(C.op() != Op::NoTrans || !C.aligned(), "unmtr_hetrd: a whole NoTrans C is required");
        if (n == 0 || C.m() == 0 || C.n() == 0) return;
        const Target target = internal::resolve_target(opts);
        const Loc loc = internal::loc_of(target);
        Matrix<T> Ag(A);
        Ag.set_uplo(Uplo::General);
        LocalBlock<T> la = Ag.local(loc, false), lt = T_[0].local(loc, false), lc = C.local(loc, true);
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        internal::unmtr_hetrd_local<T>(c, side, op, n, la.ptr, la.ld, lt.ptr, C.m(), C.n(), lc.ptr, lc.ld);
        if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
        internal::finish_origin(C, opts);
    }
}

#define SLATE_HETRD_INST(T)                                                                                   \
    template void hetrd<T>(HermitianMatrix<T>&, std::vector<real_type<T>>&, std::vector<real_type<T>>&,       \
                           TriangularFactors<T>&, Options const&);                                            \
    template void unmtr_hetrd<T>(Side, Op, HermitianMatrix<T>&, TriangularFactors<T>&, Matrix<T>&, Options const&);
SLATE_HETRD_INST(float)
SLATE_HETRD_INST(double)
SLATE_HETRD_INST(std::complex<float>)
SLATE_HETRD_INST(std::complex<double>)

}  // namespace slate
