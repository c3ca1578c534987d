// What the one-stage reductions (hetrd.cc, gebrd.cc, geqp3.cc) and their
// callers in eig.cc share on the host: the refusal of operands they cannot
// take, the event profile of a device reduction, the T factor of a panel, the
// panel-by-panel back-transform, the allocation of the T factors and the
// holder of the statistics of the last call.
#pragma once

#include "internal.hh"
#include "slate_amd/eig_host.hh"
#include "slate_amd/host_blas.hh"
#include "../kernels/kernels.hh"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace slate {
namespace internal {

static_assert(kReducePanel == slate_amd::dev::kReducePanel, "the kernels size their LDS by the panel width");

/// slate::NotImplemented unless a one-stage reduction can take this operand
/// (real type, one process, one device, block-cyclic).  `who` names the
/// routine, `what` the operand, `which` the reduction ("the one-stage
/// reduction") and `missing` what a distributed operand would need.
template <typename T>
void reduce_check_operand(BaseMatrix<T> const& A, char const* who, char const* what, char const* which,
                          char const* missing) {
    const std::string pre = std::string(who) + ": " + which + " ";
    if (is_complex_v<T>) slate_not_implemented(pre + "is implemented for real types only (" + what + " is complex)");
    if (!A.storage()) return;
    if (A.is_multi_device())
        slate_not_implemented(pre + "runs on one device (" + what + " is a multi-device matrix)");
    if (A.arbitrary_layout())
        slate_not_implemented(pre + "needs a block-cyclic operand (" + what + " has a lambda layout)");
    if (A.grid()->size() != 1)
        slate_not_implemented(pre + "needs a grid of one process (" + what + " is distributed over " +
                              std::to_string(A.grid()->size()) + "); " + missing);
}
template <typename T>
void hetrd_check_operand(BaseMatrix<T> const& A, char const* who, char const* what) {
    reduce_check_operand(A, who, what, "the one-stage reduction", "a distributed symv is not implemented");
}
template <typename T>
void gebrd_check_operand(BaseMatrix<T> const& A, char const* who, char const* what) {
    reduce_check_operand(A, who, what, "the one-stage bidiagonal reduction", "distributed products are not implemented");
}
template <typename T>
void geqp3_check_operand(BaseMatrix<T> const& A, char const* who, char const* what) {
    reduce_check_operand(A, who, what, "the QR factorization with column pivoting",
                         "the distributed pivot search is not implemented");
}

/// Statistics of the last call of a routine in this process.
template <typename S>
class LastStats {
public:
    void set(S const& s) { std::lock_guard<std::mutex> lk(mu_); v_ = s; }
    S get() { std::lock_guard<std::mutex> lk(mu_); return v_; }
private:
    std::mutex mu_;
    S v_;
};

/// With the environment variable `env` set to a nonzero number: events between
/// the kernels of a device reduction, summed per kind after the final
/// synchronisation (no extra synchronisation; the records cost a few
/// microseconds each, so the profile is for the split, not for the total).
class StageProfile {
public:
    static constexpr int Start = -1;   // the first mark: no interval ends there
    StageProfile(char const* env, int kinds, hipStream_t s) : s_(s), kinds_(kinds) {
        const char* e = std::getenv(env);
        on_ = e && std::atoi(e) != 0;
    }
    void mark(int kind) {   // the interval that ends here is of this kind
        if (!on_) return;
        hipEvent_t x;
        slate_hip_call(hipEventCreate(&x));
        slate_hip_call(hipEventRecord(x, s_));
        ev_.push_back({x, kind});
    }
    std::vector<double> finish() {   // after the stream was synchronised: milliseconds per kind
        std::vector<double> ms(size_t(kinds_), 0.0);
        for (size_t k = 1; k < ev_.size(); ++k) {
            float t = 0;
            slate_hip_call(hipEventElapsedTime(&t, ev_[k - 1].first, ev_[k].first));
            if (ev_[k].second >= 0) ms[size_t(ev_[k].second)] += t;
        }
        for (auto& x : ev_) slate_hip_call(hipEventDestroy(x.first));
        ev_.clear();
        return ms;
    }
private:
    bool on_ = false;
    hipStream_t s_ = nullptr;
    int kinds_ = 0;
    std::vector<std::pair<hipEvent_t, int>> ev_;
};

/// The T factors of a reduction of n columns, zeroed: T_[0] kReducePanel x n
/// (panel p at column p * kReducePanel), T_[1] the 1 x n tau.
template <typename T>
TriangularFactors<T> make_panel_factors(int64_t n, int64_t nb, Target target, Options const& opts) {
    const int64_t nn = std::max<int64_t>(n, 1);
    Matrix<T> Tf(nb, nn, nb, nn, Grid::self()), tau(1, nn, 1, nn, Grid::self());
    Tf.insertLocalTiles(target);
    tau.insertLocalTiles(target);
    set(T(0), T(0), Tf, opts);
    set(T(0), T(0), tau, opts);
    return TriangularFactors<T>{Tf, tau};
}

/// out (nv x kb) = the transposed row block Arow (kb x nv) of right reflectors
/// of gebrd: the unit lower trapezoid on the device, the stored entries (unit
/// entries among them, the upper triangle not read again) on the host.
template <typename R>
void form_vt(lb::Ctx const& c, int64_t nv, int64_t kb, R const* Arow, int64_t lda, R* out, int64_t ldo) {
    if (c.dev()) {
        slate_amd::dev::gebrd_form_vt<R>(nv, int(kb), Arow, lda, out, ldo, c.stream);
        return;
    }
    for (int64_t k = 0; k < kb; ++k)
        for (int64_t j = 0; j < nv; ++j) out[j + k * ldo] = Arow[k + j * lda];
}

/// T (kb x kb, leading dimension ldt) of the panel of kb reflectors of length
/// mv with the scalars tau: V in place at V (leading dimension ldv, the unit
/// lower trapezoid implied), or V == nullptr and the reflectors explicit in Vx
/// (leading dimension mv).  On the device S = V^T V by a split-K product of
/// the explicit copy in Vx (mv x kb of scratch) and the larft recurrence on S.
template <typename R>
void panel_T_factors(lb::Ctx const& c, int64_t mv, int64_t kb, R const* V, int64_t ldv, R const* tau, R* T,
                     int64_t ldt, R* Vx) {
    if (!c.dev()) {
        host::larft<R>(mv, kb, V ? V : Vx, V ? ldv : mv, tau, T, ldt);
        return;
    }
    if (V) lb::form_v(c, mv, kb, V, ldv, Vx, mv);
    lb::gemm_splitk(c, Op::Trans, Op::NoTrans, kb, kb, mv, std::max<int64_t>(1, std::min<int64_t>(32, mv / 512)), R(1),
                    Vx, mv, Vx, mv, R(0), T, ldt);
    slate_amd::dev::larft_small<R>(int(kb), tau, T, ldt, c.stream);
}

/// C (mc x nc) := op(F) C (Left) or C op(F) (Right), F = F_0 F_1 .. the nref
/// reflectors in panels of kReducePanel: the panel that starts at j0 acts on
/// the rows (columns) of C from j0 + shift on, its V is vpanel(j0, kb, ldv)
/// (which sets ldv) and its T is at Tfac + j0 * kReducePanel.  One lb::larfb
/// per panel; F C and C F^T take the panels last to first.
template <typename R, typename VPanel>
void apply_panel_reflectors(lb::Ctx const& c, Side side, Op op, int64_t nref, int64_t shift, VPanel&& vpanel,
                            R const* Tfac, int64_t mc, int64_t nc, R* C, int64_t ldc) {
    const int64_t nb = kReducePanel;
    if (nref <= 0 || mc <= 0 || nc <= 0) return;
    const int64_t np = (nref + nb - 1) / nb;
    const bool notrans = op == Op::NoTrans;
    const bool descending = (side == Side::Left) == notrans;
    const Op lop = notrans ? Op::NoTrans : Op::ConjTrans;
    for (int64_t t = 0; t < np; ++t) {
        const int64_t j0 = (descending ? np - 1 - t : t) * nb;
        const int64_t kb = std::min(nb, nref - j0), o = j0 + shift;
        int64_t ldv = 0;
        R const* V = vpanel(j0, kb, ldv);
        if (side == Side::Left) lb::larfb(c, side, lop, mc - o, nc, kb, V, ldv, Tfac + j0 * nb, nb, C + o, ldc);
        else lb::larfb(c, side, lop, mc, nc - o, kb, V, ldv, Tfac + j0 * nb, nb, C + o * ldc, ldc);
    }
}

}  // namespace internal
}  // namespace slate
