// Secular-equation arithmetic shared by the host divide-and-conquer
// (eig_host.cc stedc_secular, dc_merge.cc) and the device kernels
// (kernels/dc_merge.hip): the root finder, the pole families of the
// tridiagonal (LinearPoles) and the bidiagonal (SquaredPoles) merge, the
// strided secular sums and the z-hat entry -- one definition, compiled by
// g++ for the host and by hipcc for gfx950 (reference src/stedc_secular.cc
// calls LAPACK laed4 per root; this is the same rational "middle way"
// iteration, written from its derivation below, with a bisection safeguard).
//
// Root j of  w(lambda) = 1/rho + sum_i z_i^2 / (d_i - lambda),  d ascending,
// rho > 0, lies in (d_j, d_{j+1}) (d_k := d_{k-1} + rho |z|^2 for the last).
// It is returned as tau = lambda - d_o relative to the NEARER pole o (j or
// j + 1): the Gu-Eisenstat vectors need lambda - d_i to full relative
// precision, which the difference of two absolute values would lose.
//
// Iteration at t (shifted coordinates, delta_i = (d_i - d_o) - t): split w
// into psi (poles i <= j, left of the root) and phi (i > j), model
//   w(t + eta) ~ c + s / (delta_j - eta) + S / (delta_{j+1} - eta)
// with s = delta_j^2 psi', S = delta_{j+1}^2 phi' (derivatives matched per
// side) and c = w - delta_j psi' - delta_{j+1} phi' (value matched), and take
// the root of  c eta^2 - A eta + B = 0,
//   A = (delta_j + delta_{j+1}) w - delta_j delta_{j+1} (psi' + phi'),
//   B = delta_j delta_{j+1} w,
// in its cancellation-free form.  The model is exact for a two-pole w, so
// the step converges in a handful of iterations where the previous pure
// bisection needed 60-400 evaluations of the O(k) sum per root (the device
// merge's secular stage was 465 of 488 ms of stedc at n = 8192).  A step
// that leaves the sign bracket [a, b] falls back to bisection; the loop
// stops when |w| is at its rounding level, eps (8 (|psi| + |phi|) + 1/rho +
// |t| (psi' + phi')).
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define SLATE_SECULAR_FN __host__ __device__ inline
#else
#define SLATE_SECULAR_FN inline
#endif

namespace slate {
namespace secular {

template <typename R>
struct Sums {
    R psi = 0, phi = 0, dpsi = 0, dphi = 0;
};

/// psi / phi and their derivatives at shifted point t (origin pole o).
template <typename R>
SLATE_SECULAR_FN Sums<R> sums(int64_t k, int64_t j, const R* d, const R* z, int64_t o, R t) {
    Sums<R> s;
    const R d0 = d[o];
    for (int64_t i = 0; i <= j; ++i) {
        const R r = z[i] / ((d[i] - d0) - t);
        s.psi += z[i] * r;
        s.dpsi += r * r;
    }
    for (int64_t i = j + 1; i < k; ++i) {
        const R r = z[i] / ((d[i] - d0) - t);
        s.phi += z[i] * r;
        s.dphi += r * r;
    }
    return s;
}

/// The iteration itself, on poles known only through their differences:
/// diff(i, o) = pole_i - pole_o.  root_with passes d[i] - d[o]; the bidiagonal
/// divide and conquer has poles d_i^2 and passes the product
/// (d_i - d_o)(d_i + d_o) (SquaredPoles below), so no difference of squared
/// values is ever formed; its sum_fn builds delta_i from the same product.
template <typename R, typename DiffFn, typename SumFn>
SLATE_SECULAR_FN R root_core(int64_t k, int64_t j, R rho, R znorm2, int64_t* org, DiffFn&& diff, SumFn&& sum_fn) {
    const R eps = std::numeric_limits<R>::epsilon();
    const R rhoinv = R(1) / rho;
    const bool last = j + 1 >= k;
    const R gap = last ? rho * znorm2 : diff(j + 1, j);
    int64_t o = j;
    R a = 0, b = gap, t = gap / 2;
    if (!last) {
        // the sign of w at the midpoint picks the half, and with it the
        // nearer pole as origin
        const Sums<R> s = sum_fn(j, gap / 2);
        if (rhoinv + s.psi + s.phi < R(0)) { o = j + 1; a = -gap / 2; b = 0; t = -gap / 4; }
        else { b = gap / 2; t = gap / 4; }
    }
    const R dj0 = diff(j, o), dj1 = last ? R(0) : diff(j + 1, o);
    for (int it = 0; it < 200; ++it) {
        const Sums<R> s = sum_fn(o, t);
        const R w = rhoinv + s.psi + s.phi;
        if (w == R(0)) break;
        if (w > R(0)) b = t; else a = t;
        const R dw = s.dpsi + s.dphi;
        const R erretm = R(8) * (s.phi - s.psi) + rhoinv + std::fabs(t) * dw;
        if (std::fabs(w) <= eps * erretm) break;
        const R Dj = dj0 - t;
        R eta;
        if (!last) {
            const R Dj1 = dj1 - t;
            const R C = w - Dj * s.dpsi - Dj1 * s.dphi;
            const R A = (Dj + Dj1) * w - Dj * Dj1 * dw;
            const R B = Dj * Dj1 * w;
            const R disc = std::sqrt(std::fabs(A * A - R(4) * B * C));
            if (C == R(0)) eta = B / A;
            else if (A <= R(0)) eta = (A - disc) / (R(2) * C);
            else eta = R(2) * B / (A + disc);
        } else {
            const R C = w - Dj * s.dpsi;
            eta = Dj + Dj * Dj * s.dpsi / C;
        }
        // the step must point toward the root (w increases with t)
        if (!(w * eta < R(0))) eta = -w / dw;
        R tn = t + eta;
        if (!(tn > a && tn < b)) tn = (a + b) / 2;
        if (tn == t) break;
        t = tn;
        if (b - a <= R(2) * eps * std::fmax(std::fabs(a), std::fabs(b))) break;
    }
    *org = o;
    return t;
}

/// Root j (0-based) of the secular equation; *org receives the origin pole.
/// sum_fn(o, t) -> Sums<R> evaluates psi / phi and their derivatives (the
/// serial `sums` here; the device kernel passes a wave-parallel one, every
/// lane then runs the same iteration on the same reduced values).
template <typename R, typename SumFn>
SLATE_SECULAR_FN R root_with(int64_t k, int64_t j, R rho, const R* d, R znorm2, int64_t* org, SumFn&& sum_fn) {
    return root_core<R>(k, j, rho, znorm2, org, [d](int64_t i, int64_t o) { return d[i] - d[o]; }, sum_fn);
}

template <typename R>
SLATE_SECULAR_FN R root(int64_t k, int64_t j, R rho, const R* d, const R* z, R znorm2, int64_t* org) {
    return root_with<R>(k, j, rho, d, znorm2, org, [&](int64_t o, R t) { return sums(k, j, d, z, o, t); });
}

/// Poles d_i^2 (singular values): the converged shift t = sigma^2 - d_o^2 as
/// tau = sigma - d_o = t / (sigma + d_o), free of cancellation (the origin is
/// the nearer pole, so d_o^2 + t >= d_o^2 / 2).
template <typename R>
SLATE_SECULAR_FN R sqrt_shift(R d_o, R t) {
    const R den = std::sqrt(std::fmax(d_o * d_o + t, R(0))) + d_o;
    return den > R(0) ? t / den : R(0);
}

/// Pole families of the two merges.  Each holds the pole array d (ascending)
/// and gives, in one fixed operand order:
///   diff(i, o)                pole_i - pole_o (root_core);
///   delta(i, d0, t)           pole_i - pole_o - t with d0 = d[o], the
///                             denominator of the secular sums;
///   shift(o, t)               the converged shift as tau, root = d[o] + tau;
///   root_minus_pole(o, tau, i)   root (o, tau) minus pole i (z-hat);
///   pole_minus_root(i, dr, tr)   pole i minus root (dr = d[o], tr = tau), the
///                             denominator of a secular vector entry.
/// LinearPoles: pole d_i (stedc).
template <typename R>
struct LinearPoles {
    const R* d;
    SLATE_SECULAR_FN R diff(int64_t i, int64_t o) const { return d[i] - d[o]; }
    SLATE_SECULAR_FN R delta(int64_t i, R d0, R t) const { return (d[i] - d0) - t; }
    SLATE_SECULAR_FN R shift(int64_t, R t) const { return t; }
    SLATE_SECULAR_FN R root_minus_pole(int64_t o, R tau, int64_t i) const { return (d[o] - d[i]) + tau; }
    SLATE_SECULAR_FN R pole_minus_root(int64_t i, R dr, R tr) const { return (d[i] - dr) - tr; }
};

/// SquaredPoles: pole d_i^2, root sigma^2 (bdsdc), known only through
/// (d_i - d_o)(d_i + d_o); tau = sigma - d_o.
template <typename R>
struct SquaredPoles {
    const R* d;
    SLATE_SECULAR_FN R diff(int64_t i, int64_t o) const { return (d[i] - d[o]) * (d[i] + d[o]); }
    SLATE_SECULAR_FN R delta(int64_t i, R d0, R t) const { return (d[i] - d0) * (d[i] + d0) - t; }
    SLATE_SECULAR_FN R shift(int64_t o, R t) const { return sqrt_shift(d[o], t); }
    SLATE_SECULAR_FN R root_minus_pole(int64_t o, R tau, int64_t i) const {
        const R dorg = d[o], di = d[i];
        return ((dorg - di) + tau) * ((dorg + di) + tau);
    }
    SLATE_SECULAR_FN R pole_minus_root(int64_t i, R dr, R tr) const {
        const R di = d[i];
        return ((di - dr) - tr) * ((di + dr) + tr);
    }
};

/// The terms i = first, first + stride, ... of psi / phi and their derivatives
/// at shifted point t (origin pole o): all of them with (0, 1); a wave passes
/// (lane, 64) and adds the lanes' partial sums.
template <typename R, typename Poles>
SLATE_SECULAR_FN Sums<R> partial_sums(Poles const& p, int64_t k, int64_t j, const R* z, int64_t o, R t, int64_t first,
                                      int64_t stride) {
    Sums<R> s;
    const R d0 = p.d[o];
    for (int64_t i = first; i < k; i += stride) {
        const R r = z[i] / p.delta(i, d0, t);
        if (i <= j) { s.psi += z[i] * r; s.dpsi += r * r; }
        else { s.phi += z[i] * r; s.dphi += r * r; }
    }
    return s;
}

/// tau of root j on a pole family; sum_fn(o, t) -> Sums<R> as for root_with.
template <typename R, typename Poles, typename SumFn>
SLATE_SECULAR_FN R root_of(Poles const& p, int64_t k, int64_t j, R rho, R znorm2, int64_t* org, SumFn&& sum_fn) {
    const R t = root_core<R>(k, j, rho, znorm2, org, [p](int64_t i, int64_t o) { return p.diff(i, o); }, sum_fn);
    return p.shift(*org, t);
}

/// Entry i of z recomputed from the roots (Loewner / Gu-Eisenstat):
/// zh_i^2 = prod_j (root_j - pole_i) / (rho prod_{j != i} (pole_j - pole_i)),
/// with the sign of z_i.  The bidiagonal merge has rho = 1.
template <typename R, typename Poles>
SLATE_SECULAR_FN R zhat_entry(Poles const& p, int64_t k, int64_t i, R rho, const R* z, const int64_t* org,
                              const R* tau) {
    R pr = p.root_minus_pole(org[k - 1], tau[k - 1], i) / rho;
    // the select is on the differences, not on the index: j is uniform over a wave, so both poles are scalar loads
    for (int64_t j = 0; j < k - 1; ++j)
        pr *= p.root_minus_pole(org[j], tau[j], i) / (j < i ? p.diff(j, i) : p.diff(j + 1, i));
    return std::copysign(std::sqrt(std::fabs(pr)), z[i]);
}

}  // namespace secular
}  // namespace slate

#undef SLATE_SECULAR_FN
