// Sturm-count arithmetic shared by the host bisection (eig_host.cc
// stebz_range / sturm_counts) and the device kernels (kernels/stebz.hip): the
// count recurrence, the start interval, the stopping rules, the trial points
// of one multisection step and the index semantics -- one definition,
// compiled by g++ for the host and by hipcc for gfx950.  Written from the
// math; the reference has no such routine.
//
// T = tridiag(d, e) symmetric of order n, scaled to unit max-norm.  With
// T - x I = L D L^T the pivots are
//   q_1 = d_1 - x,   q_i = d_i - x - e_{i-1}^2 / q_{i-1},
// and by Sylvester's law of inertia N(x), the number of eigenvalues below x,
// is the number of negative q_i.  A pivot with |q| < pivmin is replaced by
// -pivmin, pivmin = safmin max(1, max e_i^2): the recurrence never divides by
// zero, e_i^2 / q stays finite, and the count is the exact count of a matrix
// within a few ulp per entry of T.  A zero e_i needs no splitting: the
// quotient vanishes and the recurrence restarts by itself.  The computed N is
// non-decreasing in x up to rounding at the eigenvalues themselves.
//
// Eigenvalue k (1-based, ascending) is bracketed by lo <= lambda_k < hi with
// N(lo) < k <= N(hi).  One multisection step puts P points inside (lo, hi),
// counts at each and keeps the subinterval whose ends have counts < k and
// >= k: the interval shrinks by P + 1 (P = 1 is bisection).  Every eigenvalue
// starts from the same interval and depends on (n, d, e, k, P) only, so a
// subset of the eigenvalues has the bits of the same entries of the full set.
//
// Singular values of an upper bidiagonal B (d, e) are the non-negative
// eigenvalues of the Golub-Kahan tridiagonal of order 2n: zero diagonal,
// off-diagonals d_1, e_1, d_2, ..., d_n.  Each entry of B enters one e^2 with
// one rounding, so the count is the exact count of a bidiagonal with entries
// changed RELATIVELY by a few ulp, which moves every singular value
// relatively by (2n - 1) times that: bisection with a relative stopping rule
// gives high relative accuracy down to the floor below.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define SLATE_STURM_FN __host__ __device__ inline
#else
#define SLATE_STURM_FN inline
#endif

namespace slate {
namespace sturm {

/// Bisection steps (P = 1) from the widest start interval of a unit max-norm
/// matrix (|gl|, |gu| <= 3, widened: below 2^3) down to floor<R>() =
/// sqrt(safmin) = 2^((min_exponent - 1) / 2): the cap that makes an exact
/// zero singular value terminate.  515 for double, 67 for float.
template <typename R>
constexpr int kStepCap = (2 - std::numeric_limits<R>::min_exponent) / 2 + 4;

/// Steps of P-point multisection never exceed this: a step shrinks the
/// interval by P + 1 >= 2^floor(log2(P + 1)).
template <typename R>
inline int step_cap(int P) {
    int bits = 0;
    while ((2 << bits) <= P + 1) ++bits;
    return kStepCap<R> / std::max(bits, 1) + 1;
}

/// Relative accuracy of the bidiagonal values ends here (times the scale):
/// below it e^2 underflows, and a value is the midpoint of its last interval.
template <typename R>
inline R floor_value() {
    return std::ldexp(R(1), (std::numeric_limits<R>::min_exponent - 1) / 2);   // safmin = 2^(min_exponent - 1)
}

/// pivmin of the scaled squares e2 (n - 1 of them)
template <typename R>
inline R pivmin_of(int64_t n, const R* e2) {
    R m = R(1);
    for (int64_t i = 0; i + 1 < n; ++i) m = std::max(m, e2[i]);
    return std::numeric_limits<R>::min() * m;
}

/// One pivot: q_i from q_{i-1}.  The first pivot is pivot(d_1, 0, 1, x).
template <typename R>
SLATE_STURM_FN R pivot(R di, R e2, R q, R x, R pivmin) {
    const R r = (di - x) - e2 / q;
    return (r < pivmin && r > -pivmin) ? -pivmin : r;
}

/// N(x): e2[i] = e_i^2 couples rows i and i + 1.
template <typename R>
SLATE_STURM_FN int64_t count(int64_t n, const R* d, const R* e2, R x, R pivmin) {
    int64_t c = 0;
    R q = R(1);
    for (int64_t i = 0; i < n; ++i) {
        q = pivot(d[i], i > 0 ? e2[i - 1] : R(0), q, x, pivmin);
        c += q < R(0);
    }
    return c;
}

template <typename R>
struct Interval {
    R lo = 0, hi = 0;
};

/// Start interval: Gershgorin of the whole matrix (e: the n - 1 off-diagonal
/// entries, any sign), widened by 2 n eps max(|gl|, |gu|) + 2 pivmin.
template <typename R>
inline Interval<R> start_interval(int64_t n, const R* d, const R* e, R pivmin) {
    Interval<R> iv;
    if (n <= 0) return iv;
    R gl = d[0], gu = d[0];
    for (int64_t i = 0; i < n; ++i) {
        const R r = (i > 0 ? std::abs(e[i - 1]) : R(0)) + (i + 1 < n ? std::abs(e[i]) : R(0));
        gl = std::min(gl, d[i] - r);
        gu = std::max(gu, d[i] + r);
    }
    const R w = R(2) * R(n) * std::numeric_limits<R>::epsilon() * std::max(std::abs(gl), std::abs(gu)) + R(2) * pivmin;
    iv.lo = gl - w;
    iv.hi = gu + w;
    return iv;
}

/// What ends the refinement of one interval.
///   tridiagonal: abstol = eps max|T_ij| (eps after scaling), floor = 0:
///     hi - lo <= 2 eps max(|lo|, |hi|) + abstol, absolute accuracy;
///   bidiagonal:  abstol = 0, floor = floor_value():
///     hi - lo <= 2 eps max(|lo|, |hi|), relative accuracy, or the whole
///     interval at or below the floor.
template <typename R>
struct Stop {
    R abstol = 0, floor = 0;
};

template <typename R>
SLATE_STURM_FN bool converged(R lo, R hi, Stop<R> st) {
    const R alo = lo < 0 ? -lo : lo, ahi = hi < 0 ? -hi : hi;
    const R m = alo > ahi ? alo : ahi;
    return hi - lo <= R(2) * std::numeric_limits<R>::epsilon() * m + st.abstol || m <= st.floor;
}

/// Trial point p (0 .. P - 1) of a step on [lo, hi].
template <typename R>
SLATE_STURM_FN R point(R lo, R hi, int p, int P) {
    return lo + (hi - lo) * (R(p + 1) / R(P + 1));
}

/// The value returned for a final interval.
template <typename R>
SLATE_STURM_FN R value_of(R lo, R hi) {
    return lo + (hi - lo) * R(0.5);
}

/// Plain bisection (P = 1) for eigenvalue k (0-based, ascending) from iv:
/// the host twin of the device step.  Returns the steps taken.
template <typename R>
inline int bisect(int64_t n, const R* d, const R* e2, int64_t k, Interval<R> iv, R pivmin, Stop<R> st, R* value) {
    R lo = iv.lo, hi = iv.hi;
    int steps = 0;
    const int cap = step_cap<R>(1);
    while (!converged(lo, hi, st) && steps < cap) {
        const R x = point(lo, hi, 0, 1);
        if (count(n, d, e2, x, pivmin) <= k) lo = x;   // N(x) < k + 1: lambda_k >= x
        else hi = x;
        ++steps;
    }
    *value = value_of(lo, hi);
    return steps;
}

/// Index semantics.  Eigenvalues wanted are the ascending 0-based [k0, k1).
///   Index: 1-based il <= k <= iu            -> [il - 1, iu)
///   Value: N(vl) < k <= N(vu) (1-based)     -> [N(vl), N(vu)), never below
///          kmin (bdsbz keeps the upper half of the Golub-Kahan spectrum).
struct Wanted {
    int64_t k0 = 0, k1 = 0;
};
SLATE_STURM_FN Wanted wanted_of_counts(int64_t cl, int64_t cu, int64_t kmin) {
    Wanted w;
    w.k0 = cl > kmin ? cl : kmin;
    w.k1 = cu > w.k0 ? cu : w.k0;
    return w;
}

}  // namespace sturm
}  // namespace slate
