// One-stage bidiagonal reduction (LAPACK gebrd: labrd panels plus two gemm
// updates, written from the math) and its back-transforms (ormbr), real types,
// m >= n, upper bidiagonal, on ONE contiguous local array of either target.
//
// Each column makes two dependent passes over the trailing matrix, A^T u and
// then A v: on the device both read the block once per product
// (kernels/gebrd.hip), the panel steps are multi-workgroup kernels whose
// reductions are two-level and deterministic, and d, e, tauq, taup stay on the
// device: the only host synchronisation is the one that fetches d and e at the
// end.  The trailing updates are two lb::gemm, the T factors S = V^T V plus the
// larft recurrence (for P on the transposed row block), the back-transforms one
// lb::larfb per panel.  The host target runs host::gebrd (eig_host.cc), the
// same algorithm in plain loops.
#include "reduce_common.hh"

namespace slate {

namespace {
internal::LastStats<GebrdStats> g_stats;   // of the last reduction in this process
}  // namespace

GebrdStats gebrd_stats() { return g_stats.get(); }

namespace lb {

template <typename R>
void gemv_block(Ctx const& c, Op op, int64_t mr, int64_t nc, R const* A, int64_t lda, R const* x, R* y) {
    if (mr <= 0 || nc <= 0) return;
    slate_error_if_msg(!c.dev(), "gemv_block: a device product");
    namespace kd = slate_amd::dev;
    Scratch sc(c);
    if (op == Op::NoTrans) {
        R* work = sc.alloc<R>(size_t(kd::gemv_n_block_workspace(mr, nc)));
        kd::gemv_n_block<R>(mr, nc, A, lda, x, y, work, c.stream);
    } else {
        R* work = sc.alloc<R>(size_t(kd::gemv_t_block_workspace(mr, nc)));
        kd::gemv_t_block<R>(mr, nc, A, lda, x, y, work, c.stream);
    }
}
template void gemv_block<float>(Ctx const&, Op, int64_t, int64_t, float const*, int64_t, float const*, float*);
template void gemv_block<double>(Ctx const&, Op, int64_t, int64_t, double const*, int64_t, double const*, double*);

}  // namespace lb

namespace internal {

namespace {
/// SLATE_GEBRD_PROFILE=1 (StageProfile): the kinds of GebrdStats::ms_*
enum GebrdKind { Panel = 0, Pass1 = 1, Pass2 = 2, Gemm = 3, Larft = 4, Kinds = 5 };
}  // namespace

template <typename R>
void gebrd_local(lb::Ctx const& c, int64_t m, int64_t n, R* A, int64_t lda, std::vector<R>& d, std::vector<R>& e,
                 R* tauq, R* taup, R* TQ, R* TP) {
    namespace kd = slate_amd::dev;
    const int64_t nb = kGebrdPanel;
    slate_error_if_msg(m < n, "gebrd: m >= n is required");
    d.assign(n, R(0));
    e.assign(std::max<int64_t>(n - 1, 0), R(0));
    if (n == 0) return;
    GebrdStats st;
    // T factors: every panel's reflectors are final (later panels touch A(k1:, k1:) only); P's from
    // the transposed row block, explicit in Vx
    Work<R> Vx(c.dev() ? Target::Devices : Target::Host, size_t(m) * nb);
    auto t_factors = [&]() {
        for (int64_t j0 = 0; j0 < n; j0 += nb) {
            panel_T_factors<R>(c, m - j0, std::min(nb, n - j0), A + j0 + j0 * lda, lda, tauq + j0, TQ + j0 * nb, nb,
                               Vx.data());
            const int64_t kp = std::min(nb, n - 1 - j0), nv = n - j0 - 1;
            if (kp <= 0) continue;
            form_vt<R>(c, nv, kp, A + j0 + (j0 + 1) * lda, lda, Vx.data(), nv);
            panel_T_factors<R>(c, nv, kp, nullptr, 0, taup + j0, TP + j0 * nb, nb, Vx.data());
        }
    };
    if (!c.dev()) {
        std::vector<R> eh(n, R(0));
        host::gebrd<R>(m, n, A, lda, d.data(), eh.data(), tauq, taup, nb);
        std::copy(eh.begin(), eh.begin() + (n - 1), e.begin());
        t_factors();
        st.panels = (n + nb - 1) / nb;
        st.columns = n;
        g_stats.set(st);
        return;
    }
    hipStream_t s = c.stream;
    const int64_t mx = std::max(m, n);
    const int64_t ndot = (mx + 255) / 256, nrm = (m + 63) / 64, nrn = (n + 63) / 64;
    Work<R> XY(Target::Devices, size_t(m + n) * nb), vec(Target::Devices, size_t(m) + 5 * n + 2 + nrm + nrn + 128 * ndot);
    const size_t ncolpart = size_t(m / 256 + 2) * n, nrowpart = size_t(n / 16 + 2) * m;
    Work<R> part(Target::Devices, ncolpart + nrowpart);
    kd::GebrdWork<R> wk;
    wk.X = XY.data(); wk.ldx = m;
    wk.Y = XY.data() + size_t(m) * nb; wk.ldy = n;
    R* p = vec.data();
    wk.u = p; p += m;
    wk.v = p; p += n;
    wk.d = p; p += n;
    wk.e = p; p += n;
    wk.scal = p; p += 2;
    wk.ssq = p; p += nrm;
    wk.ssq2 = p; p += nrn;
    wk.pdots = p;
    wk.tauq = tauq;
    wk.taup = taup;
    wk.colpart = part.data();
    wk.rowpart = part.data() + ncolpart;
    StageProfile prof("SLATE_GEBRD_PROFILE", Kinds, s);
    prof.mark(StageProfile::Start);
    for (int64_t j0 = 0; j0 < n; j0 += nb) {
        const int64_t kb = std::min(nb, n - j0), k1 = j0 + kb;
        {
            trace::Block tp("gebrd_panel");
            for (int64_t i = j0; i < k1; ++i) {
                kd::gebrd_column<R>(m, i, j0, A, lda, wk, s);
                kd::gebrd_larfg_u<R>(m, i, A, lda, wk, s);
                ++st.launches_column;
                ++st.launches_larfg_u;
                if (i == n - 1) { prof.mark(Panel); break; }
                prof.mark(Panel);
                kd::gebrd_pass1<R>(m, n, i, j0, A, lda, wk, s);
                prof.mark(Pass1);
                kd::gebrd_finish_y<R>(m, n, i, j0, A, lda, wk, s);
                kd::gebrd_larfg_v<R>(n, i, A, lda, wk, s);
                prof.mark(Panel);
                kd::gebrd_pass2<R>(m, n, i, j0, A, lda, wk, s);
                prof.mark(Pass2);
                kd::gebrd_finish_x<R>(m, n, i, j0, A, lda, wk, s);
                ++st.launches_pass1;
                ++st.launches_finish_y;
                ++st.launches_larfg_v;
                ++st.launches_pass2;
                ++st.launches_finish_x;
            }
            prof.mark(Panel);
        }
        st.columns += kb;
        ++st.panels;
        if (k1 < n) {
            trace::Block tu("gebrd_gemm");
            lb::gemm(c, Op::NoTrans, Op::Trans, m - k1, n - k1, kb, R(-1), A + k1 + j0 * lda, lda, wk.Y + k1, wk.ldy,
                     R(1), A + k1 + k1 * lda, lda);
            lb::gemm(c, Op::NoTrans, Op::NoTrans, m - k1, n - k1, kb, R(-1), wk.X + k1, wk.ldx, A + j0 + k1 * lda, lda,
                     R(1), A + k1 + k1 * lda, lda);
            prof.mark(Gemm);
        }
    }
    {
        trace::Block tt("gebrd_larft");
        t_factors();
        prof.mark(Larft);
    }
    device::memcpy_async(d.data(), wk.d, size_t(n) * sizeof(R), s);
    if (n > 1) device::memcpy_async(e.data(), wk.e, size_t(n - 1) * sizeof(R), s);
    slate_hip_call(hipStreamSynchronize(s));
    st.host_syncs = 1;
    const std::vector<double> ms = prof.finish();
    st.ms_panel = ms[Panel]; st.ms_pass1 = ms[Pass1]; st.ms_pass2 = ms[Pass2]; st.ms_gemm = ms[Gemm];
    st.ms_larft = ms[Larft];
    g_stats.set(st);
}

template <typename R>
void unmbr_gebrd_local(lb::Ctx const& c, Vect vect, Side side, Op op, int64_t m, int64_t n, R const* A, int64_t lda,
                       R const* Tfac, int64_t mc, int64_t nc, R* C, int64_t ldc) {
    const int64_t nb = kGebrdPanel;
    const bool q = vect == Vect::Q;
    const int64_t order = q ? m : n, nref = q ? n : n - 1;   // reflectors
    slate_error_if_msg((side == Side::Left ? mc : nc) != order,
                       q ? "unmbr_gebrd: C does not match Q" : "unmbr_gebrd: C does not match P");
    Work<R> Vt(c.dev() ? Target::Devices : Target::Host, q || nref <= 0 ? size_t(1) : size_t(n) * nb);
    apply_panel_reflectors<R>(c, side, op, nref, q ? 0 : 1, [&](int64_t j0, int64_t kb, int64_t& ldv) -> R const* {
        if (q) {
            ldv = lda;
            return A + j0 + j0 * lda;
        }
        // the transposed row block A(j0:j0+kb, j0+1:n), explicit
        ldv = n - j0 - 1;
        form_vt<R>(c, ldv, kb, A + j0 + (j0 + 1) * lda, lda, Vt.data(), ldv);
        return Vt.data();
    }, Tfac, mc, nc, C, ldc);
}

#define SLATE_GEBRD_LOCAL_INST(R)                                                                                 \
    template void gebrd_local<R>(lb::Ctx const&, int64_t, int64_t, R*, int64_t, std::vector<R>&, std::vector<R>&, \
                                 R*, R*, R*, R*);                                                                 \
    template void unmbr_gebrd_local<R>(lb::Ctx const&, Vect, Side, Op, int64_t, int64_t, R const*, int64_t,       \
                                       R const*, int64_t, int64_t, R*, int64_t);
SLATE_GEBRD_LOCAL_INST(float)
SLATE_GEBRD_LOCAL_INST(double)

}  // namespace internal

//------------------------------------------------------------------------------
template <typename T>
void gebrd(Matrix<T>& A, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E, TriangularFactors<T>& TQ,
           TriangularFactors<T>& TP, Options const& opts) {
    trace::Block tb("gebrd");
    internal::DriverScope ds_;
    internal::gebrd_check_operand<T>(A, "gebrd", "A");
    if (A.m() < A.n())
        slate_not_implemented("gebrd: the one-stage bidiagonal reduction needs m >= n (A is " +
                              std::to_string(A.m()) + " x " + std::to_string(A.n()) + "); reduce the transpose");
    if constexpr (!is_complex_v<T>) {
        slate_error_if_msg(A.op() != Op::NoTrans || !A.aligned(), "gebrd: a whole NoTrans matrix is required");
        const Target target = internal::resolve_target(opts);
        const int64_t m = A.m(), n = A.n(), nb = internal::kGebrdPanel;
        TQ = internal::make_panel_factors<T>(n, nb, target, opts);
        TP = internal::make_panel_factors<T>(n, nb, target, opts);
        D.assign(n, T(0));
        E.assign(std::max<int64_t>(n - 1, 0), T(0));
        if (n == 0) return;
        const Loc loc = internal::loc_of(target);
        LocalBlock<T> la = A.local(loc, true);
        LocalBlock<T> lq = TQ[0].local(loc, true), lp = TP[0].local(loc, true);
        LocalBlock<T> ltq = TQ[1].local(loc, true), ltp = TP[1].local(loc, true);
        slate_error_if_msg(la.m != m || la.n != n || lq.ld != nb || lp.ld != nb, "gebrd: unexpected local layout");
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        internal::gebrd_local<T>(c, m, n, la.ptr, la.ld, D, E, ltq.ptr, ltp.ptr, lq.ptr, lp.ptr);
        internal::finish_origin(A, opts);
    }
}

template <typename T>
void unmbr_gebrd(Vect vect, Side side, Op op, Matrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& C,
                 Options const& opts) {
    trace::Block tb("unmbr_gebrd");
    internal::DriverScope ds_;
    internal::gebrd_check_operand<T>(A, "unmbr_gebrd", "A");
    internal::gebrd_check_operand<T>(C, "unmbr_gebrd", "C");
    if constexpr (!is_complex_v<T>) {
        const int64_t m = A.m(), n = A.n(), nb = internal::kGebrdPanel;
        slate_error_if_msg(vect != Vect::Q && vect != Vect::P, "unmbr_gebrd: vect is Vect::Q or Vect::P");
        slate_error_if_msg(m < n || A.op() != Op::NoTrans || !A.aligned(), "unmbr_gebrd: A as gebrd left it");
        slate_error_if_msg(T_.empty() || T_[0].m() != nb || T_[0].n() < n, "unmbr_gebrd: T is not from gebrd");
        slate_error_if_msg(C.op() != Op::NoTrans || !C.aligned(), "unmbr_gebrd: a whole NoTrans C is required");
        if (n == 0 || C.m() == 0 || C.n() == 0) return;
        const Target target = internal::resolve_target(opts);
        const Loc loc = internal::loc_of(target);
        LocalBlock<T> la = A.local(loc, false), lt = T_[0].local(loc, false), lc = C.local(loc, true);
        lb::Ctx c = target == Target::Devices ? lb::Ctx::device(0) : lb::Ctx::host();
        internal::unmbr_gebrd_local<T>(c, vect, side, op, m, n, la.ptr, la.ld, lt.ptr, C.m(), C.n(), lc.ptr, lc.ld);
        if (c.dev()) slate_hip_call(hipStreamSynchronize(c.stream));
        internal::finish_origin(C, opts);
    }
}

#define SLATE_GEBRD_INST(T)                                                                                  \
    template void gebrd<T>(Matrix<T>&, std::vector<real_type<T>>&, std::vector<real_type<T>>&,               \
                           TriangularFactors<T>&, TriangularFactors<T>&, Options const&);                    \
    template void unmbr_gebrd<T>(Vect, Side, Op, Matrix<T>&, TriangularFactors<T>&, Matrix<T>&, Options const&);
SLATE_GEBRD_INST(float)
SLATE_GEBRD_INST(double)
SLATE_GEBRD_INST(std::complex<float>)
SLATE_GEBRD_INST(std::complex<double>)

}  // namespace slate
