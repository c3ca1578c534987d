// Sturm-count bisection on the device (src/stebz.cc; the arithmetic is
// slate_amd/sturm.hh, shared with the host twin in eig_host.cc): eigenvalues
// of a symmetric tridiagonal, and through the Golub-Kahan form the singular
// values of a bidiagonal, from d and e^2 alone.
//
// Kernels (float and double):
//   * sturm_count: N(x_j) for an array of shifts, one lane per shift.  Every
//     lane of a wave walks i = 1 .. n in lockstep, so d_i and e_i^2 are
//     wave-uniform: the wave stages them through LDS in chunks of kSturmChunk
//     entries (n is not bounded by LDS) and every lane reads the same word
//     (an LDS broadcast).
//   * stebz_refine: the whole refinement of the wanted eigenvalues in ONE
//     launch.  A workgroup is one wave; lane = (eigenvalue, trial point):
//     the wave holds 64 / P eigenvalues with P points each.  Per step every
//     lane counts at its point, the P counts of an eigenvalue are compared
//     with k by one ballot, and the two points that bracket the eigenvalue
//     become the new [lo, hi] by two wave shuffles.  An eigenvalue that has
//     met its stopping rule keeps its interval; the wave leaves the loop when
//     all of its eigenvalues have (a wave-uniform vote), or at the step cap.
//     Eigenvalues are independent from the start interval on, so there is no
//     dependency between workgroups at all: no flags, no atomics, nothing to
//     spin on.  The range by value reads its two counts N(vl), N(vu) from
//     device memory, written by a sturm_count launch before it (a kernel
//     boundary), so the host learns the number of values from the one fetch
//     of the result.
// The division is the chain: a step is n dependent IEEE divisions per lane.
// P > 1 spends idle SIMDs on cutting the number of steps (log_{P+1} instead
// of log_2) when there are fewer eigenvalues than lanes on the device.
#include "device_common.hh"
#include "kernels.hh"

namespace slate_amd {
namespace dev {

namespace {

constexpr int kSturmChunk = 512;   // d and e^2 entries per LDS stage

/// entries [base, base + len) of d and of the e^2 that precedes each row
template <typename R>
__device__ inline void stage(int64_t base, int len, const R* __restrict__ d, const R* __restrict__ e2, R* sd, R* se,
                             int lane) {
    for (int t = lane; t < len; t += kWave) {
        const int64_t i = base + t;
        sd[t] = d[i];
        se[t] = i > 0 ? e2[i - 1] : R(0);
    }
}

template <typename R>
__device__ inline void walk(int len, const R* sd, const R* se, R x, R pivmin, R& q, int64_t& c) {
    #pragma unroll 4
    for (int t = 0; t < len; ++t) {
        q = slate::sturm::pivot(sd[t], se[t], q, x, pivmin);
        c += q < R(0);
    }
}

/// N(x) of this lane's x; all 64 lanes of the workgroup (one wave) take part.
/// staged: the whole matrix (n <= kSturmChunk) is already in sd / se.
template <typename R>
__device__ inline int64_t count_wave(int64_t n, const R* __restrict__ d, const R* __restrict__ e2, R x, R pivmin,
                                     R* sd, R* se, int lane, bool staged) {
    int64_t c = 0;
    R q = R(1);
    if (staged) {
        walk(int(n), sd, se, x, pivmin, q, c);
        return c;
    }
    for (int64_t base = 0; base < n; base += kSturmChunk) {
        const int len = int(n - base < kSturmChunk ? n - base : kSturmChunk);
        __syncthreads();   // the previous chunk has been walked
        stage(base, len, d, e2, sd, se, lane);
        __syncthreads();
        walk(len, sd, se, x, pivmin, q, c);
    }
    return c;
}

template <typename R>
__global__ __launch_bounds__(kWave) void sturm_count_kernel(int64_t n, const R* __restrict__ d,
                                                            const R* __restrict__ e2, R pivmin, int64_t nx,
                                                            const R* __restrict__ x, int64_t* __restrict__ cnt) {
    __shared__ R sd[kSturmChunk], se[kSturmChunk];
    const int lane = threadIdx.x;
    const int64_t j = int64_t(blockIdx.x) * kWave + lane;
    const R xj = j < nx ? x[j] : R(0);   // idle lanes walk along: the barriers are the wave's
    const int64_t c = count_wave(n, d, e2, xj, pivmin, sd, se, lane, false);
    if (j < nx) cnt[j] = c;
}

template <typename R>
__global__ __launch_bounds__(kWave) void stebz_refine_kernel(StebzRefine<R> a) {
    __shared__ R sd[kSturmChunk], se[kSturmChunk];
    const int lane = threadIdx.x;
    const int P = a.points, G = kWave / P;
    const int g = lane / P, p = lane - g * P;
    int64_t k0 = a.k0, k1 = a.k1;
    if (a.cnt) {
        const slate::sturm::Wanted w = slate::sturm::wanted_of_counts(a.cnt[0], a.cnt[1], a.kmin);
        k0 = w.k0;
        k1 = w.k1;
    }
    const int64_t kfirst = k0 + int64_t(blockIdx.x) * G;
    if (kfirst >= k1) return;   // wave-uniform: the workgroup is this wave
    const int64_t k = kfirst + g;
    const bool valid = k < k1;
    const bool staged = a.n <= kSturmChunk;
    if (staged) {
        stage(int64_t(0), int(a.n), a.d, a.e2, sd, se, lane);
        __syncthreads();
    }
    const slate::sturm::Stop<R> stop{a.abstol, a.floor};
    R lo = a.lo, hi = a.hi;
    int steps = 0;
    bool done = !valid || slate::sturm::converged(lo, hi, stop);
    const unsigned long long gmask = P == kWave ? ~0ull : ((1ull << P) - 1ull);
    for (int it = 0; it < a.max_steps; ++it) {
        if (!__any(!done)) break;   // wave-uniform
        const R x = slate::sturm::point(lo, hi, p, P);
        const int64_t c = count_wave(a.n, a.d, a.e2, x, a.pivmin, sd, se, lane, staged);
        // points at or below lambda_k: N(x) < k + 1
        const unsigned long long below = __ballot(c <= k);
        const int j = __popcll((below >> (g * P)) & gmask);
        const R xl = __shfl(x, g * P + (j > 0 ? j - 1 : 0));
        const R xh = __shfl(x, g * P + (j < P ? j : P - 1));
        if (!done) {
            if (j > 0) lo = xl;
            if (j < P) hi = xh;
            ++steps;
            done = slate::sturm::converged(lo, hi, stop);
        }
    }
    if (valid && p == 0) {
        a.w[k - k0] = slate::sturm::value_of(lo, hi);
        a.steps[k - k0] = steps;
    }
}

}  // namespace

template <typename R>
void sturm_count(int64_t n, const R* d, const R* e2, R pivmin, int64_t nx, const R* x, int64_t* cnt, hipStream_t s) {
    if (nx <= 0) return;
    hipLaunchKernelGGL(sturm_count_kernel<R>, dim3((unsigned)((nx + kWave - 1) / kWave)), dim3(kWave), 0, s, n, d, e2,
                       pivmin, nx, x, cnt);
}

template <typename R>
void stebz_refine(StebzRefine<R> const& a, int64_t max_values, hipStream_t s) {
    if (max_values <= 0) return;
    const int G = kWave / a.points;
    hipLaunchKernelGGL(stebz_refine_kernel<R>, dim3((unsigned)((max_values + G - 1) / G)), dim3(kWave), 0, s, a);
}

template void sturm_count<float>(int64_t, const float*, const float*, float, int64_t, const float*, int64_t*,
                                 hipStream_t);
template void sturm_count<double>(int64_t, const double*, const double*, double, int64_t, const double*, int64_t*,
                                  hipStream_t);
template void stebz_refine<float>(StebzRefine<float> const&, int64_t, hipStream_t);
template void stebz_refine<double>(StebzRefine<double> const&, int64_t, hipStream_t);

}  // namespace dev
}  // namespace slate_amd
