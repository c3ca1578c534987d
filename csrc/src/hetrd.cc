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
#include "internal.hh"
#include "slate_amd/eig_host.hh"
#include "slate_amd/host_blas.hh"
#include "../kernels/kernels.hh"

#include <algorithm>
#include <cstdlib>
#include <mutex>

namespace slate {

namespace {
std::mutex g_stats_mu;
HetrdStats g_stats;   // of the last reduction in this process
}  // namespace

HetrdStats hetrd_stats() {
    std::lock_guard<std::mutex> lk(g_stats_mu);
    return g_stats;
}

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

/// SLATE_HETRD_PROFILE=1: events between the kernels of the device reduction,
/// summed per kind into HetrdStats::ms_* after the final synchronisation (no
/// extra synchronisation; the records cost a few microseconds each, so the
/// profile is for the split, not for the total).
struct HetrdProfile {
    enum Kind { Start = -1, Panel = 0, Symv = 1, Syr2k = 2, Larft = 3 };
    bool on = false;
    hipStream_t s = nullptr;
    std::vector<std::pair<hipEvent_t, int>> ev;
    HetrdProfile(hipStream_t st) : s(st) {
        const char* e = std::getenv("SLATE_HETRD_PROFILE");
        on = e && std::atoi(e) != 0;
    }
    void mark(int kind) {   // the interval that ends here is of this kind
        if (!on) return;
        hipEvent_t x;
        slate_hip_call(hipEventCreate(&x));
        slate_hip_call(hipEventRecord(x, s));
        ev.push_back({x, kind});
    }
    void finish(HetrdStats& st) {   // after the stream was synchronised
        double ms[4] = {0, 0, 0, 0};
        for (size_t k = 1; k < ev.size(); ++k) {
            float t = 0;
            slate_hip_call(hipEventElapsedTime(&t, ev[k - 1].first, ev[k].first));
            if (ev[k].second >= 0) ms[ev[k].second] += t;
        }
        for (auto& x : ev) slate_hip_call(hipEventDestroy(x.first));
        ev.clear();
        st.ms_panel = ms[Panel]; st.ms_symv = ms[Symv]; st.ms_syr2k = ms[Syr2k]; st.ms_larft = ms[Larft];
    }
};

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
    if (!c.dev()) {
        std::vector<R> eh(n, R(0));
        host::hetrd<R>(n, A, lda, d.data(), eh.data(), tau, nb);
        std::copy(eh.begin(), eh.begin() + (n - 1), e.begin());
        for (int64_t j0 = 0; j0 < n - 1; j0 += nb) {
            const int64_t kb = std::min(nb, n - 1 - j0);
            host::larft<R>(n - j0 - 1, kb, A + (j0 + 1) + j0 * lda, lda, tau + j0, Tfac + j0 * nb, nb);
            ++st.panels;
            st.columns += kb;
        }
        std::lock_guard<std::mutex> lk(g_stats_mu);
        g_stats = st;
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
    HetrdProfile prof(s);
    prof.mark(HetrdProfile::Start);
    for (int64_t j0 = 0; j0 < n - 1; j0 += nb) {
        const int64_t kb = std::min(nb, n - 1 - j0), k1 = j0 + kb;
        {
            trace::Block tp("hetrd_panel");
            for (int64_t i = j0; i < k1; ++i) {
                kd::hetrd_column<R>(n, i, j0, true, A, lda, wk, s);
                kd::hetrd_larfg<R>(n, i, A, lda, wk, s);
                prof.mark(HetrdProfile::Panel);
                kd::hetrd_symv<R>(n, i, j0, A, lda, wk, s);
                prof.mark(HetrdProfile::Symv);
                kd::hetrd_correct<R>(n, i, j0, A, lda, wk, s);
            }
            kd::hetrd_column<R>(n, k1, j0, false, A, lda, wk, s);   // last column of W
            prof.mark(HetrdProfile::Panel);
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
        prof.mark(HetrdProfile::Syr2k);
    }
    device::memcpy_async(wk.d + (n - 1), A + (n - 1) + (n - 1) * lda, sizeof(R), s);
    {
        // T factors: every panel's V is final (later panels touch A(k1:, k1:) only)
        trace::Block tt("hetrd_larft");
        Work<R> Vx(Target::Devices, size_t(n) * nb);
        for (int64_t j0 = 0; j0 < n - 1; j0 += nb) {
            const int64_t kb = std::min(nb, n - 1 - j0), mv = n - j0 - 1;
            R* Tp = Tfac + j0 * nb;
            lb::form_v(c, mv, kb, A + (j0 + 1) + j0 * lda, lda, Vx.data(), mv);
            lb::gemm_splitk(c, Op::Trans, Op::NoTrans, kb, kb, mv, std::max<int64_t>(1, std::min<int64_t>(32, mv / 512)),
                            R(1), Vx.data(), mv, Vx.data(), mv, R(0), Tp, nb);
            kd::larft_small<R>(int(kb), tau + j0, Tp, nb, s);
        }
        prof.mark(HetrdProfile::Larft);
    }
    device::memcpy_async(d.data(), wk.d, size_t(n) * sizeof(R), s);
    if (n > 1) device::memcpy_async(e.data(), wk.e, size_t(n - 1) * sizeof(R), s);
    slate_hip_call(hipStreamSynchronize(s));
    st.host_syncs = 1;
    prof.finish(st);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_stats = st;
}

template <typename R>
void unmtr_hetrd_local(lb::Ctx const& c, Side side, Op op, int64_t n, R const* A, int64_t lda, R const* Tfac,
                       int64_t mc, int64_t nc, R* C, int64_t ldc) {
    const int64_t nb = kHetrdPanel;
    slate_error_if_msg((side == Side::Left ? mc : nc) != n, "unmtr_hetrd: C does not match Q");
    if (n < 2 || mc <= 0 || nc <= 0) return;
    const int64_t np = (n - 1 + nb - 1) / nb;
    // Q = Q_0 Q_1 .. Q_{np-1}: Q C and C Q^T take the panels last to first
    const bool notrans = op == Op::NoTrans;
    const bool descending = (side == Side::Left) == notrans;
    for (int64_t t = 0; t < np; ++t) {
        const int64_t j0 = (descending ? np - 1 - t : t) * nb;
        const int64_t kb = std::min(nb, n - 1 - j0), o = j0 + 1;
        R const* V = A + o + j0 * lda;
        if (side == Side::Left)
            lb::larfb(c, side, notrans ? Op::NoTrans : Op::ConjTrans, mc - o, nc, kb, V, lda, Tfac + j0 * nb, nb, C + o,
                      ldc);
        else
            lb::larfb(c, side, notrans ? Op::NoTrans : Op::ConjTrans, mc, nc - o, kb, V, lda, Tfac + j0 * nb, nb,
                      C + o * ldc, ldc);
    }
}

#define SLATE_HETRD_LOCAL_INST(R)                                                                              \
    template void hetrd_local<R>(lb::Ctx const&, int64_t, R*, int64_t, std::vector<R>&, std::vector<R>&, R*, R*); \
    template void unmtr_hetrd_local<R>(lb::Ctx const&, Side, Op, int64_t, R const*, int64_t, R const*, int64_t, \
                                       int64_t, R*, int64_t);
SLATE_HETRD_LOCAL_INST(float)
SLATE_HETRD_LOCAL_INST(double)

template <typename T>
void hetrd_check_operand(BaseMatrix<T> const& A, char const* who, char const* what) {
    const std::string pre = std::string(who) + ": the one-stage reduction ";
    if (is_complex_v<T>) slate_not_implemented(pre + "is implemented for real types only (" + what + " is complex)");
    if (!A.storage()) return;
    if (A.is_multi_device())
        slate_not_implemented(pre + "runs on one device (" + what + " is a multi-device matrix)");
    if (A.arbitrary_layout())
        slate_not_implemented(pre + "needs a block-cyclic operand (" + what + " has a lambda layout)");
    if (A.grid()->size() != 1)
        slate_not_implemented(pre + "needs a grid of one process (" + what + " is distributed over " +
                              std::to_string(A.grid()->size()) + "); a distributed symv is not implemented");
}
#define SLATE_HETRD_CHECK_INST(T) template void hetrd_check_operand<T>(BaseMatrix<T> const&, char const*, char const*);
SLATE_HETRD_CHECK_INST(float)
SLATE_HETRD_CHECK_INST(double)
SLATE_HETRD_CHECK_INST(std::complex<float>)
SLATE_HETRD_CHECK_INST(std::complex<double>)

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
        Matrix<T> Tf(nb, std::max<int64_t>(n, 1), nb, std::max<int64_t>(n, 1), Grid::self());
        Matrix<T> tau(1, std::max<int64_t>(n, 1), 1, std::max<int64_t>(n, 1), Grid::self());
        Tf.insertLocalTiles(target);
        tau.insertLocalTiles(target);
        set(T(0), T(0), Tf, opts);
        set(T(0), T(0), tau, opts);
        T_.clear();
        T_.push_back(Tf);
        T_.push_back(tau);
        D.assign(n, T(0));
        E.assign(std::max<int64_t>(n - 1, 0), T(0));
        if (n == 0) return;
        const Loc loc = internal::loc_of(target);
        LocalBlock<T> la = Ag.local(loc, true), lt = Tf.local(loc, true), ltau = tau.local(loc, true);
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
