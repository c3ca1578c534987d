// Inverse-iteration arithmetic shared by the host twin (eig_host.cc
// host::stein) and the device kernels (kernels/stein.hip): the pivoted
// factorization of T - lambda I, the two solves, the start vector, the
// clusters and the acceptance rule -- one definition, compiled by g++ for the
// host and by hipcc for gfx950.  Written from the math, with the structure of
// LAPACK's stein / lagtf / lagts; the reference has no such routine.
//
// T = tridiag(d, e) symmetric of order n, scaled to unit max-norm, lambda one
// of its computed eigenvalues.  One round for one vector:
//   * forward: T - lambda I = P L U with partial pivoting between adjacent
//     rows (lagtf).  U has three diagonals (ua, ub, ud).  Row k of U is final
//     once rows k and k + 1 have been compared, so the factorization and the
//     forward solve y = L^-1 P^T b run in one sweep i = 0 .. n - 1 that
//     carries one pending row; nothing of L is kept, the sweep is repeated
//     every round (two multiplications and a division per row, against the
//     four stores the row costs anyway).  The pivot choice is a select.
//   * backward: x = U^-1 y (lagts, job = -1): a pivot too small for its
//     numerator is pushed away from zero by tol = eps max|U|, doubled until
//     the quotient cannot overflow; the doubling is capped (kPertCap), and
//     at the cap the pivot has modulus >= 1, which always passes.
//   * the right-hand side is scaled to |b|_inf = n |T|_1 eps, the smallest
//     scale LAPACK's rule n |T|_1 max(eps, |u_nn|) / |b|_inf can give; the
//     solve is linear, so the growth LAPACK tests is that of this solve times
//     max(eps, |u_nn|) / eps: accepted means
//       |x|_inf max(eps, |u_nn|) / eps >= sqrt(0.1 / n)
//     in three rounds (the first that passes and two further ones).  (LAPACK's
//     code divides by the entry of largest modulus, |b|_inf; so does this.)
// Eigenvalues closer than 1e-3 |T|_1 chain into a cluster, whose vectors are
// orthonormalised against each other in value order after every round.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define SLATE_STEIN_FN __host__ __device__ inline
#else
#define SLATE_STEIN_FN inline
#endif

namespace slate {
namespace invit {

constexpr int kRounds = 5;     // LAPACK's MAXITS: every call runs exactly this many
constexpr int kAccept = 3;     // passes of the growth test that finish a vector (EXTRA + 1)

/// Doublings of the pivot replacement never exceed this: tol >= the smallest
/// subnormal, and a pivot of modulus >= 1 passes.
template <typename R>
constexpr int kPertCap = std::numeric_limits<R>::max_exponent - std::numeric_limits<R>::min_exponent +
                         std::numeric_limits<R>::digits + 8;

template <typename R>
SLATE_STEIN_FN R absv(R x) { return x < R(0) ? -x : x; }

/// Entry `row` of the start vector of eigenvalue number `index`: a hash
/// (splitmix64's finaliser) of the pair, uniform in [-1, 1).  No state.
template <typename R>
SLATE_STEIN_FN R start_entry(int64_t row, int64_t index) {
    uint64_t z = uint64_t(row) * 0x9E3779B97F4A7C15ull + uint64_t(index) * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return R(int64_t(z >> 40) - (int64_t(1) << 23)) * R(1.0 / 8388608.0);   // 24 bits: exact in float
}

/// The pending row of the forward sweep: pivot candidate a, superdiagonal b,
/// right-hand side y of row k, the scale of row k (lagtf's scale1) and the
/// largest modulus in U so far.
template <typename R>
struct Fwd {
    R a, b, y, scale, umax;
};

/// Row 0 pending: d0 - lambda, e0 (0 when n = 1), b_0.
template <typename R>
SLATE_STEIN_FN Fwd<R> fwd_start(R d0, R e0, R lambda, R y0) {
    Fwd<R> s;
    s.a = d0 - lambda;
    s.b = e0;
    s.y = y0;
    s.scale = absv(s.a) + absv(s.b);
    s.umax = R(0);
    return s;
}

/// Rows k and k + 1: dk1 = d_{k+1}, ck = e_k (the coupling of the two rows),
/// bk1 = e_{k+1} (0 for the last row), yk1 the right-hand side of row k + 1.
/// Returns row k of U and of y; row k + 1 becomes the pending row.
template <typename R>
SLATE_STEIN_FN void fwd_step(Fwd<R>& s, R lambda, R dk1, R ck, R bk1, R yk1, R& ua, R& ub, R& ud, R& yk) {
    const R a1 = dk1 - lambda;
    const R scale2 = absv(ck) + absv(a1) + absv(bk1);
    // |ck| / scale2 > |a| / scale: the larger relative pivot moves up
    const bool swap = ck != R(0) && (s.a == R(0) || absv(ck) * s.scale > absv(s.a) * scale2);
    const R num = swap ? s.a : ck, den = swap ? ck : s.a;
    const R mult = ck == R(0) ? R(0) : num / den;
    ua = swap ? ck : s.a;
    ub = swap ? a1 : s.b;
    ud = swap ? bk1 : R(0);
    yk = swap ? yk1 : s.y;
    const R na = swap ? s.b - mult * a1 : a1 - mult * s.b;
    const R nb = swap ? -mult * bk1 : bk1;
    const R ny = swap ? s.y - mult * yk1 : yk1 - mult * s.y;
    s.a = na;
    s.b = nb;
    s.y = ny;
    s.scale = swap ? s.scale : scale2;
    const R m1 = absv(ua) > absv(ub) ? absv(ua) : absv(ub);
    const R m2 = m1 > absv(ud) ? m1 : absv(ud);
    s.umax = s.umax > m2 ? s.umax : m2;
}

/// The last row: U's (ua, 0, 0) and y are the pending row itself.
template <typename R>
SLATE_STEIN_FN void fwd_finish(Fwd<R>& s, R& ua, R& yk) {
    ua = s.a;
    yk = s.y;
    s.umax = s.umax > absv(ua) ? s.umax : absv(ua);
}

/// tol of the back substitution from max|U|.
template <typename R>
SLATE_STEIN_FN R back_tol(R umax) {
    const R t = umax * std::numeric_limits<R>::epsilon();
    return t > R(0) ? t : std::numeric_limits<R>::epsilon();
}

/// x_k = (y_k - ub x_{k+1} - ud x_{k+2}) / ua with lagts' replacement of a
/// pivot that would overflow the quotient.
template <typename R>
SLATE_STEIN_FN R back_step(R ua, R ub, R ud, R yk, R x1, R x2, R tol) {
    const R sfmin = std::numeric_limits<R>::min();
    const R bignum = R(1) / sfmin;
    R temp = yk - ub * x1 - ud * x2;
    R ak = ua;
    R pert = ak < R(0) ? -tol : tol;
    for (int it = 0; it < kPertCap<R>; ++it) {
        const R aa = absv(ak), at = absv(temp);
        const bool grow = aa < R(1) && (aa < sfmin ? (aa == R(0) || at * sfmin > aa) : at > aa * bignum);
        if (!grow) break;
        ak += pert;
        pert += pert;
    }
    if (absv(ak) < sfmin) {   // passed: |temp| sfmin <= |ak|, the scaled quotient is finite
        temp *= bignum;
        ak *= bignum;
    }
    return temp / ak;
}

/// LAPACK's growth test on the solve of the minimally scaled right-hand side.
template <typename R>
SLATE_STEIN_FN bool grown(R xinf, R unn, int64_t n) {
    const R eps = std::numeric_limits<R>::epsilon();
    const R g = absv(unn) > eps ? absv(unn) / eps : R(1);
    return absv(xinf) * g >= std::sqrt(R(0.1) / R(n));
}

/// |b|_inf of the scaled right-hand side: n |T|_1 eps.
template <typename R>
inline R rhs_norm(int64_t n, R onenrm) {
    return R(n) * onenrm * std::numeric_limits<R>::epsilon();
}

/// |T|_1 of the scaled matrix.
template <typename R>
inline R one_norm(int64_t n, const R* d, const R* e) {
    R m = R(0);
    for (int64_t i = 0; i < n; ++i)
        m = std::max(m, std::abs(d[i]) + (i > 0 ? std::abs(e[i - 1]) : R(0)) + (i + 1 < n ? std::abs(e[i]) : R(0)));
    return m;
}

/// Clusters of the scaled ascending values w (m of them), fixed on the host
/// before the first launch.  Consecutive values closer than 1e-3 |T|_1 chain;
/// a value is moved up until it is 10 eps |lambda| above its predecessor
/// (LAPACK's PERTOL).  cluster[j] is the number of j's cluster or -1 for a
/// value on its own; first / last (inclusive) delimit cluster c.
template <typename R>
struct Clusters {
    std::vector<int32_t> cluster;
    std::vector<int64_t> first, last;
    int64_t largest = 0;
};

template <typename R>
inline Clusters<R> find_clusters(int64_t m, R* w, R onenrm) {
    Clusters<R> c;
    c.cluster.assign(size_t(m), -1);
    const R ortol = R(1e-3) * onenrm, eps = std::numeric_limits<R>::epsilon();
    for (int64_t j = 1; j < m; ++j) {
        const R pertol = R(10) * std::abs(eps * w[j]);
        if (w[j] - w[j - 1] < pertol) w[j] = w[j - 1] + pertol;
        if (w[j] - w[j - 1] < ortol) {
            if (c.cluster[j - 1] < 0) {
                c.cluster[j - 1] = int32_t(c.first.size());
                c.first.push_back(j - 1);
                c.last.push_back(j - 1);
            }
            c.cluster[j] = c.cluster[j - 1];
            c.last.back() = j;
        }
    }
    for (size_t k = 0; k < c.first.size(); ++k) c.largest = std::max(c.largest, c.last[k] - c.first[k] + 1);
    return c;
}

/// One round of one vector on arrays of its own (stride 1: the host twin).
/// x: the iterate in, the solution out; ua, ub, ud: n reals of scratch each.
/// bscale = rhs_norm / |x|_inf of the iterate (|x|_inf taken as 1 in round 0,
/// where x is the start vector).
/// Returns u_nn; xmax is the entry of largest modulus (the first of equals,
/// signed) and sumsq the sum of squares of the solution.
template <typename R>
inline R solve_round(int64_t n, const R* d, const R* e, R lambda, R bscale, R* x, R* ua, R* ub, R* ud, R& xmax,
                     R& sumsq) {
    Fwd<R> s = fwd_start<R>(d[0], n > 1 ? e[0] : R(0), lambda, x[0] * bscale);
    for (int64_t k = 0; k + 1 < n; ++k)
        fwd_step<R>(s, lambda, d[k + 1], e[k], k + 2 < n ? e[k + 1] : R(0), x[k + 1] * bscale, ua[k], ub[k], ud[k],
                    x[k]);
    fwd_finish<R>(s, ua[n - 1], x[n - 1]);
    ub[n - 1] = ud[n - 1] = R(0);
    const R unn = ua[n - 1], tol = back_tol<R>(s.umax);
    R x1 = R(0), x2 = R(0);
    xmax = R(0);
    sumsq = R(0);
    for (int64_t k = n - 1; k >= 0; --k) {
        const R xk = back_step<R>(ua[k], ub[k], ud[k], x[k], x1, x2, tol);
        x[k] = xk;
        x2 = x1;
        x1 = xk;
        if (absv(xk) >= absv(xmax)) xmax = xk;   // descending k: the first of equals wins
        sumsq += xk * xk;
    }
    return unn;
}

}  // namespace invit
}  // namespace slate
