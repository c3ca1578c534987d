// Tridiagonal eigenvectors by inverse iteration on the device (src/stein.cc;
// the arithmetic is slate_amd/stein.hh, shared with the host twin host::stein
// in eig_host.cc).
//
// Kernels (float and double):
//   * stein_solve: one round of every vector, one lane per eigenvector, a
//     workgroup is one wave.  The lanes walk i = 0 .. n - 1 in lockstep, so
//     d_i and e_i are wave-uniform and staged through LDS in chunks of
//     kSteinChunk entries (n is not bounded by LDS).  The forward sweep
//     factors T - lambda I and solves with L in one pass and writes row i of U
//     (three diagonals) and of y; the backward sweep reads them and writes x
//     over y.  All four arrays are laid out [row][vector], so a wave reads
//     and writes 64 consecutive elements at every step.  The pivot choice is
//     a select.  Round 0 takes its right-hand side from the hash of
//     (row, vector) instead of memory.  A finished vector's lane walks along
//     without storing; a wave with no unfinished vector leaves at once.
//   * stein_orth: one workgroup of 256 per cluster; the columns in value
//     order, each by classical Gram-Schmidt applied twice against the columns
//     before it, taken 256 at a time.  The dot products of a block are summed
//     per column over row groups, the partials through LDS in a fixed order;
//     norms and the entry of largest modulus by a fixed tree.  No atomics.
//     O(n c^2) on one CU for a cluster of c values.
//   * stein_transpose: [row][vector] into column-major Z through an LDS tile,
//     with the scaling to unit norm and the sign of the largest entry.
// Every dependency between workgroups is a kernel boundary.
#include "device_common.hh"
#include "kernels.hh"

namespace slate_amd {
namespace dev {

namespace {

namespace st = slate::invit;

constexpr int kSteinChunk = 512;   // rows per LDS stage
constexpr int kOrthThreads = 256;
constexpr int kTile = 64;
static_assert(kSteinLanes == kWave, "one lane per eigenvector: the workspaces are padded to the wave");

template <typename R>
__global__ __launch_bounds__(kWave) void stein_solve_kernel(SteinSolve<R> a) {
    __shared__ R sd[kSteinChunk], se[kSteinChunk + 1];
    const int lane = threadIdx.x;
    const int64_t j = int64_t(blockIdx.x) * kWave + lane;
    const int64_t n = a.n, mp = a.mp;
    const bool active = j < a.m && a.done[j] == 0;
    if (!__any(active)) return;   // wave-uniform: the workgroup is this wave
    const int64_t jj = j < a.m ? j : a.m - 1;
    const R lambda = a.w[jj];
    const bool first = a.round == 0;
    R scale = a.bnorm;
    if (!first) {
        const R xm = st::absv(a.xmax[jj]);
        scale = xm > R(0) ? a.bnorm / xm : a.bnorm;
    }
    R* x = a.x + j;
    R* ua = a.ua + j;
    R* ub = a.ub + j;
    R* ud = a.ud + j;
    // forward: step k compares rows k and k + 1
    st::Fwd<R> s = st::fwd_start<R>(a.d[0], n > 1 ? a.e[0] : R(0), lambda,
                                    (first ? st::start_entry<R>(0, j) : x[0]) * scale);
    for (int64_t base = 0; base + 1 < n; base += kSteinChunk) {
        const int len = int(n - 1 - base < kSteinChunk ? n - 1 - base : kSteinChunk);
        __syncthreads();   // the previous chunk has been walked
        for (int t = lane; t <= len; t += kWave) {
            const int64_t i = base + t;
            if (t < len) sd[t] = a.d[i + 1];
            se[t] = i < n - 1 ? a.e[i] : R(0);
        }
        __syncthreads();
        for (int t = 0; t < len; ++t) {
            const int64_t k = base + t;
            const R yk1 = (first ? st::start_entry<R>(k + 1, j) : x[(k + 1) * mp]) * scale;
            R va, vb, vd, vy;
            st::fwd_step<R>(s, lambda, sd[t], se[t], se[t + 1], yk1, va, vb, vd, vy);
            if (active) {
                ua[k * mp] = va;
                ub[k * mp] = vb;
                ud[k * mp] = vd;
                x[k * mp] = vy;
            }
        }
    }
    R unn, yn;
    st::fwd_finish<R>(s, unn, yn);
    const R tol = st::back_tol<R>(s.umax);
    // backward
    R x1 = st::back_step<R>(unn, R(0), R(0), yn, R(0), R(0), tol), x2 = R(0);
    if (active) x[(n - 1) * mp] = x1;
    R xmax = x1, sumsq = x1 * x1;
    for (int64_t k = n - 2; k >= 0; --k) {
        const R xk = st::back_step<R>(ua[k * mp], ub[k * mp], ud[k * mp], x[k * mp], x1, x2, tol);
        if (active) x[k * mp] = xk;
        x2 = x1;
        x1 = xk;
        if (st::absv(xk) >= st::absv(xmax)) xmax = xk;
        sumsq += xk * xk;
    }
    if (active) {
        a.unn[j] = unn;
        a.xmax[j] = xmax;
        a.nrm[j] = sqrt(sumsq);
        if (a.cluster[j] < 0) {   // a vector of a cluster is judged after the orthonormalisation
            const int32_t p = a.pass[j] + (st::grown<R>(xmax, unn, n) ? 1 : 0);
            a.pass[j] = p;
            a.done[j] = p >= st::kAccept ? 1 : 0;
        }
    }
}

/// the sum of v over the workgroup in a fixed tree; every thread gets it
template <typename R>
__device__ inline R block_sum(R v, R* red, int t) {
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int h = kOrthThreads / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    return red[0];
}

/// the entry of largest modulus over the workgroup (the lower thread of equals); every thread gets it
template <typename R>
__device__ inline R block_absmax(R v, R* red, int t) {
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int h = kOrthThreads / 2; h > 0; h >>= 1) {
        if (t < h && st::absv(red[t + h]) > st::absv(red[t])) red[t] = red[t + h];
        __syncthreads();
    }
    return red[0];
}

template <typename R>
__global__ __launch_bounds__(kOrthThreads) void stein_orth_kernel(SteinOrth<R> a) {
    __shared__ R red[kOrthThreads], sh[kOrthThreads];
    const int t = threadIdx.x;
    const int64_t n = a.n, mp = a.mp;
    const int64_t j0 = a.first[blockIdx.x], j1 = a.last[blockIdx.x];
    if (a.done[j0] != 0) return;   // uniform: a cluster finishes as a whole
    R* X = a.x;
    bool ok = true;
    for (int64_t j = j0; j <= j1; ++j) {
        const int64_t np = j - j0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int64_t ib = 0; ib < np; ib += kOrthThreads) {
                const int cnt = int(np - ib < kOrthThreads ? np - ib : kOrthThreads);
                int P = 1;
                while (P < cnt) P <<= 1;
                const int G = kOrthThreads / P, i = t % P, g = t / P;
                // h_i = q_i . x: lanes across the columns i, row groups g
                R acc = R(0);
                if (i < cnt) {
                    const R* q = X + (j0 + ib + i);
                    for (int64_t r = g; r < n; r += G) acc += q[r * mp] * X[r * mp + j];
                }
                __syncthreads();
                red[t] = acc;
                __syncthreads();
                if (t < P) {
                    R sum = R(0);
                    for (int gg = 0; gg < G; ++gg) sum += red[gg * P + t];
                    sh[t] = sum;
                }
                __syncthreads();
                // x -= sum_i h_i q_i: one thread per row
                for (int64_t r = t; r < n; r += kOrthThreads) {
                    const R* q = X + r * mp + (j0 + ib);
                    R sum = R(0);
                    for (int c = 0; c < cnt; ++c) sum += sh[c] * q[c];
                    X[r * mp + j] -= sum;
                }
                __syncthreads();
            }
        }
        R lmax = R(0), lss = R(0);
        for (int64_t r = t; r < n; r += kOrthThreads) {
            const R v = X[r * mp + j];
            lss += v * v;
            if (st::absv(v) > st::absv(lmax)) lmax = v;
        }
        const R nrm = sqrt(block_sum(lss, red, t));
        const R xmax = block_absmax(lmax, red, t);
        ok = ok && st::grown<R>(xmax, a.unn[j], n);
        const R rs = nrm > R(0) ? R(1) / nrm : R(1);
        for (int64_t r = t; r < n; r += kOrthThreads) X[r * mp + j] *= rs;
        if (t == 0) {
            a.xmax[j] = xmax * rs;
            a.nrm[j] = R(1);
        }
        __syncthreads();   // column j is final before column j + 1 reads it
    }
    const int32_t cp = a.cpass[blockIdx.x] + (ok ? 1 : 0);
    __syncthreads();       // every thread has read cpass and done[j0]
    if (t == 0) a.cpass[blockIdx.x] = cp;
    if (cp >= st::kAccept)
        for (int64_t j = j0 + t; j <= j1; j += kOrthThreads) a.done[j] = 1;
}

template <typename R>
__global__ __launch_bounds__(kTile * 4) void stein_transpose_kernel(int64_t n, int64_t m, int64_t mp,
                                                                   const R* __restrict__ x,
                                                                   const R* __restrict__ xmax,
                                                                   const R* __restrict__ nrm, R* __restrict__ Z,
                                                                   int64_t ldz) {
    __shared__ R tile[kTile][kTile + 1];
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int64_t jb = int64_t(blockIdx.x) * kTile, rb = int64_t(blockIdx.y) * kTile;
    for (int rr = ty; rr < kTile; rr += 4) {
        const int64_t r = rb + rr, j = jb + tx;
        R v = R(0);
        if (r < n && j < m) {
            const R nj = nrm[j];
            const R s = (nj > R(0) ? R(1) / nj : R(1)) * (xmax[j] < R(0) ? R(-1) : R(1));
            v = x[r * mp + j] * s;
        }
        tile[rr][tx] = v;
    }
    __syncthreads();
    for (int jj = ty; jj < kTile; jj += 4) {
        const int64_t r = rb + tx, j = jb + jj;
        if (r < n && j < m) Z[r + j * ldz] = tile[tx][jj];
    }
}

}  // namespace

template <typename R>
void stein_solve(SteinSolve<R> const& a, hipStream_t s) {
    if (a.n <= 0 || a.m <= 0) return;
    hipLaunchKernelGGL(stein_solve_kernel<R>, dim3((unsigned)(a.mp / kWave)), dim3(kWave), 0, s, a);
}

template <typename R>
void stein_orth(SteinOrth<R> const& a, int64_t clusters, hipStream_t s) {
    if (a.n <= 0 || clusters <= 0) return;
    hipLaunchKernelGGL(stein_orth_kernel<R>, dim3((unsigned)clusters), dim3(kOrthThreads), 0, s, a);
}

template <typename R>
void stein_transpose(int64_t n, int64_t m, int64_t mp, const R* x, const R* xmax, const R* nrm, R* Z, int64_t ldz,
                     hipStream_t s) {
    if (n <= 0 || m <= 0) return;
    const int64_t rt = (n + kTile - 1) / kTile, ct = (m + kTile - 1) / kTile;
    // rows in blockIdx.y: at most 65535 tiles a launch
    for (int64_t r0 = 0; r0 < rt; r0 += 65535) {
        const int64_t nr = std::min<int64_t>(65535, rt - r0);
        const int64_t row0 = r0 * kTile;
        hipLaunchKernelGGL(stein_transpose_kernel<R>, dim3((unsigned)ct, (unsigned)nr), dim3(kTile * 4), 0, s,
                           std::min<int64_t>(n - row0, nr * kTile), m, mp, x + row0 * mp, xmax, nrm, Z + row0, ldz);
    }
}

#define SLATE_STEIN_KERNEL_INST(R)                                                                       \
    template void stein_solve<R>(SteinSolve<R> const&, hipStream_t);                                     \
    template void stein_orth<R>(SteinOrth<R> const&, int64_t, hipStream_t);                              \
    template void stein_transpose<R>(int64_t, int64_t, int64_t, const R*, const R*, const R*, R*, int64_t, \
                                     hipStream_t);
SLATE_STEIN_KERNEL_INST(float)
SLATE_STEIN_KERNEL_INST(double)

}  // namespace dev
}  // namespace slate_amd
