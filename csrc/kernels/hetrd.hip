// Device side of the one-stage tridiagonal reduction (src/hetrd.cc; LAPACK's
// sytrd / latrd, written from the math), real types, lower triangle.
//
// Column i of a panel that starts at j0 (c = i - j0, V = A(:, j0:i), W the
// n x nb workspace) takes four launches, every dependency between workgroups
// being a kernel boundary (no flags, no waiting, no atomics):
//   1 hetrd_column   w of column i-1 finished (scaled by tau, corrected with
//                    w^T v), A(i:n, i) -= V W(i,:)^T + W V(i,:)^T, d_i, and
//                    per-workgroup sums of squares of A(i+2:n, i)
//   2 hetrd_larfg    beta, tau from those sums; v scaled in place, unit entry
//                    stored, v copied to a contiguous vector (larfg_vec.hip)
//   3 hetrd_symv     partials of A(i+1:n, i+1:n) v from the lower triangle,
//                    and in the same grid the partials of V^T v and W^T v
//   4 hetrd_correct  partials summed in a fixed order, w -= V (W^T v) +
//                    W (V^T v), per-workgroup partials of w^T v
// Every reduction has two levels: partials go to a workspace, and each
// workgroup of the next kernel sums them again in the same order, so all
// workgroups see the same bits and two runs give identical results.  The block
// reductions, the small dots V^T v and W^T v and their gather are those of
// gebrd.hip and geqp3.hip: reduce_tiles.hh.
//
// symv_lower: the block is cut into tiles of 64 rows x 16 columns.  A lane
// owns one row of a tile (a wave reads 64 consecutive elements of a column:
// coalesced whatever the alignment of the block's base, which is only
// element-aligned and moves every column), keeps the row sum y_I += A_IJ x_J
// and 16 column partials for y_J += A_IJ^T x_I.  A workgroup takes one block
// column and 4 x tpw row tiles; its waves take different tiles, so the column
// partials stay in registers over the tiles and are reduced once, and each
// tile's row sums go out as they are (the reduction of the column partials is
// gemv_t_tiles': reduce_tiles.hh).  The tile on the diagonal masks its loads:
// the strict upper triangle is never read.
#include "device_common.hh"
#include "reduce_tiles.hh"
#include "kernels.hh"

#include <algorithm>

namespace slate_amd {
namespace dev {

namespace {

// GT, TR, TC, GR, KP, the gb_* reductions, gb_larfg, panel_dots and gather_pdots: reduce_tiles.hh

// chunks of row tiles that block column J of an order-m block has
__device__ inline int64_t symv_chunks_of(int64_t m, int tpw, int64_t J) {
    const int64_t nrt = (m + TR - 1) / TR - (J * TC) / TR;
    return (nrt + 4 * tpw - 1) / (4 * tpw);
}

// one workgroup of the symv: block column J, chunk k
template <typename R>
__device__ inline void symv_tiles(int64_t m, const R* A, int64_t lda, const R* x, R* rowpart, R* colpart, int tpw,
                                  int64_t k, int64_t J, R* cbuf) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = J * TC;
    const int nc = int(min(int64_t(TC), m - c0));
    const int64_t nRT = (m + TR - 1) / TR;
    const int64_t tbase = c0 / TR + k * (4 * tpw);
    if (tbase >= nRT) return;   // uniform over the workgroup
    R xc[TC], cacc[TC];
    #pragma unroll
    for (int c = 0; c < TC; ++c) {
        xc[c] = c < nc ? x[c0 + c] : R(0);
        cacc[c] = R(0);
    }
    for (int s = 0; s < tpw; ++s) {
        const int64_t t = tbase + w + 4 * s;
        if (t >= nRT) break;    // uniform over the wave
        const int64_t r = t * TR + lane;
        const bool inb = r < m;
        const R* ap = A + r + c0 * lda;
        const R xr = inb ? x[r] : R(0);
        R racc = R(0);
        // columns c <= lim of this row are stored; lim >= TC below the diagonal tile
        const int lim = inb ? int(min(r - c0, int64_t(TC))) : -1;
        const int ldlim = min(lim, nc - 1);
        #pragma unroll
        for (int c = 0; c < TC; ++c) {
            // a masked lane loads x[0] instead (a valid address) and drops it: no branch per load
            const R ld = *(c <= ldlim ? ap + c * lda : x);
            const R a = c <= ldlim ? ld : R(0);
            racc += a * xc[c];
            cacc[c] += c < lim ? a * xr : R(0);
        }
        if (inb) rowpart[J * m + r] = racc;
    }
    gb_colpart_reduce<R>(cacc, nc, colpart + k * m + c0, cbuf);
}

// wave g's share of y_i of the symv from its partials, in a fixed order
template <typename R>
__device__ inline R symv_gather(int64_t m, int tpw, const R* rowpart, const R* colpart, int64_t i, int g) {
    const int64_t nJ = (m + TC - 1) / TC;
    const int64_t jend = min(nJ, (TR / TC) * (i / TR + 1));   // block columns whose first row tile is at or above row i's
    R s = R(0);
    #pragma unroll 4
    for (int64_t J = g; J < jend; J += 4) s += rowpart[J * m + i];
    const int64_t kend = symv_chunks_of(m, tpw, i / TC);
    for (int64_t k = g; k < kend; k += 4) s += colpart[k * m + i];
    return s;
}

template <typename R>
__global__ __launch_bounds__(GT) void symv_lower_kernel(int64_t m, const R* A, int64_t lda, const R* x,
                                                           R* rowpart, R* colpart, int tpw) {
    __shared__ R cbuf[4 * TC * 65];
    symv_tiles<R>(m, A, lda, x, rowpart, colpart, tpw, blockIdx.x, blockIdx.y, cbuf);
}

template <typename R>
__global__ __launch_bounds__(GT) void symv_reduce_kernel(int64_t m, const R* rowpart, const R* colpart, int tpw,
                                                         R* y) {
    __shared__ R red[4][GR];
    const int64_t i = int64_t(blockIdx.x) * GR + (threadIdx.x & 63);
    const R v = gb_waves_sum<R>(i < m ? symv_gather<R>(m, tpw, rowpart, colpart, i, threadIdx.x >> 6) : R(0), red);
    if (i < m && threadIdx.x < 64) y[i] = v;
}

//------------------------------------------------------------------------------
// 1: rows r >= i.  c > 0: column c-1 of W finished from wraw, tau_{i-1} and
// the partials of wraw^T v.  update: column i of A updated, d_i, alpha and the
// partial sums of squares below it.
template <typename R>
__global__ __launch_bounds__(GT) void hetrd_column_kernel(int64_t n, int64_t i, int64_t j0, int update, R* A,
                                                          int64_t lda, HetrdWork<R> wk, int npdot) {
    __shared__ R sh[4];
    __shared__ R Wi[KP], Vi[KP];
    __shared__ R red[4][GR];
    const int c = int(i - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t r = i + int64_t(blockIdx.x) * GR + lane;
    const bool inb = r < n;
    R wfin = R(0), tau_p = R(0), a2 = R(0);
    if (c > 0) {
        tau_p = wk.tau[i - 1];
        a2 = R(0.5) * tau_p * tau_p * gb_partial_sum<R>(wk.pdot, npdot, sh);
        if (inb) {
            wfin = tau_p * wk.wraw[r] - a2 * wk.v[r];
            if (g == 0) wk.W[r + int64_t(c - 1) * wk.ldw] = wfin;
        }
    }
    if (!update) return;
    if (int(threadIdx.x) < c) {
        const int k = threadIdx.x;
        // W(i, c-1) is being written by the workgroup that owns row i: form it here
        Wi[k] = k == c - 1 ? tau_p * wk.wraw[i] - a2 * wk.v[i] : wk.W[i + int64_t(k) * wk.ldw];
        Vi[k] = A[i + (j0 + k) * lda];
    }
    __syncthreads();
    R s = R(0);
    if (inb) {
        #pragma unroll 4
        for (int k = g; k < c; k += 4) {
            const R wv = k == c - 1 ? wfin : wk.W[r + int64_t(k) * wk.ldw];
            s += A[r + (j0 + k) * lda] * Wi[k] + wv * Vi[k];
        }
    }
    s = gb_waves_sum<R>(s, red);
    R a = R(0);
    if (inb && g == 0) {
        a = A[r + i * lda] - s;
        A[r + i * lda] = a;
        if (r == i) wk.d[i] = a;
        if (r == i + 1) wk.scal[0] = a;
    }
    const R ss = gb_block_sum<R>(g == 0 && inb && r >= i + 2 ? a * a : R(0), sh);
    if (threadIdx.x == 0) wk.ssq[blockIdx.x] = ss;
}

// 3: symv partials of the trailing block with v, and (blockIdx.y >= nJ) the
// partials of V^T v and W^T v over 256 rows each, one wave per column
template <typename R>
__global__ __launch_bounds__(GT) void hetrd_symv_kernel(int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda,
                                                        HetrdWork<R> wk, int tpw, int nJ, int ndots) {
    __shared__ R cbuf[4 * TC * 65];
    const int64_t o = i + 1, m = n - o;
    if (int(blockIdx.y) < nJ) {
        symv_tiles<R>(m, A + o + o * lda, lda, wk.v + o, wk.rowpart, wk.colpart, tpw, blockIdx.x, blockIdx.y, cbuf);
        return;
    }
    const int64_t q = int64_t(blockIdx.y - nJ) * gridDim.x + blockIdx.x;
    if (q >= ndots) return;
    panel_dots<R, true>(o + q * GT, n, wk.v, int(i - j0), A + j0 * lda, lda, wk.W, wk.ldw, wk.pvw + q * (2 * KP));
}

// 4: rows r >= i+1.  wraw = A v - V (W^T v) - W (V^T v), partials of wraw^T v
template <typename R>
__global__ __launch_bounds__(GT) void hetrd_correct_kernel(int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda,
                                                           HetrdWork<R> wk, int tpw, int ndots) {
    __shared__ R sh[4];
    __shared__ R tvw[2 * KP];   // V^T v | W^T v
    __shared__ R red[4][GR];
    const int c = int(i - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    gather_pdots<R>(wk.pvw, ndots, 2 * KP, c, c, tvw);
    __syncthreads();
    const int64_t o = i + 1, m = n - o;
    const int64_t r = o + int64_t(blockIdx.x) * GR + lane;
    R part = R(0);
    if (r < n) {
        part = symv_gather<R>(m, tpw, wk.rowpart, wk.colpart, r - o, g);
        R s = R(0);
        #pragma unroll 4
        for (int k = g; k < c; k += 4)
            s += A[r + (j0 + k) * lda] * tvw[KP + k] + wk.W[r + int64_t(k) * wk.ldw] * tvw[k];
        part -= s;
    }
    const R wr = gb_waves_sum<R>(part, red);
    R p = R(0);
    if (r < n && g == 0) {
        wk.wraw[r] = wr;
        p = wr * wk.v[r];
    }
    p = gb_block_sum<R>(p, sh);
    if (threadIdx.x == 0) wk.pdot[blockIdx.x] = p;
}

}  // namespace

int symv_lower_tpw(int64_t m) {
    const int64_t nRT = (m + TR - 1) / TR, nJ = (m + TC - 1) / TC;
    const int64_t tiles = nJ * (nRT + 1) / 2;
    return int(std::max<int64_t>(1, std::min<int64_t>(8, tiles / (4 * 512))));
}
int64_t symv_lower_chunks(int64_t m, int tpw) {
    return std::max<int64_t>(1, ((m + TR - 1) / TR + 4 * tpw - 1) / (4 * tpw));
}
int64_t symv_lower_workspace(int64_t m) {
    const int tpw = symv_lower_tpw(m);
    return std::max<int64_t>(1, ((m + TC - 1) / TC + symv_lower_chunks(m, tpw)) * m);
}

template <typename R>
void symv_lower(int64_t m, const R* A, int64_t lda, const R* x, R* y, R* work, hipStream_t s) {
    if (m <= 0) return;
    const int tpw = symv_lower_tpw(m);
    const int64_t nJ = (m + TC - 1) / TC, nk = symv_lower_chunks(m, tpw);
    R* rowpart = work;
    R* colpart = work + nJ * m;
    hipLaunchKernelGGL(symv_lower_kernel<R>, dim3(unsigned(nk), unsigned(nJ)), dim3(GT), 0, s, m, A, lda, x, rowpart,
                       colpart, tpw);
    hipLaunchKernelGGL(symv_reduce_kernel<R>, dim3(grblocks_of(m)), dim3(GT), 0, s, m, rowpart, colpart, tpw, y);
}

template <typename R>
void hetrd_column(int64_t n, int64_t i, int64_t j0, bool update, R* A, int64_t lda, HetrdWork<R> const& wk,
                  hipStream_t s) {
    if (i >= n) return;
    const unsigned g = grblocks_of(n - i);
    hipLaunchKernelGGL(hetrd_column_kernel<R>, dim3(g), dim3(GT), 0, s, n, i, j0, update ? 1 : 0, A, lda, wk, int(g));
}
template <typename R>
void hetrd_larfg(int64_t n, int64_t i, R* A, int64_t lda, HetrdWork<R> const& wk, hipStream_t s) {
    larfg_vec<R>(n - i - 1, A + (i + 1) + i * lda, 1, wk.scal, wk.ssq, int(grblocks_of(n - i)), wk.tau + i, wk.e + i,
                 wk.v + i + 1, false, s);
}
template <typename R>
void hetrd_symv(int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda, HetrdWork<R> const& wk, hipStream_t s) {
    const int64_t m = n - i - 1;
    const int tpw = symv_lower_tpw(m);
    const int64_t nJ = (m + TC - 1) / TC, nk = symv_lower_chunks(m, tpw);
    const int64_t ndots = i > j0 ? gblocks_of(m) : 0;
    hipLaunchKernelGGL(hetrd_symv_kernel<R>, product_grid(nk, nJ, ndots), dim3(GT), 0, s, n, i, j0, A, lda, wk, tpw,
                       int(nJ), int(ndots));
}
template <typename R>
void hetrd_correct(int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda, HetrdWork<R> const& wk, hipStream_t s) {
    const int64_t m = n - i - 1;
    hipLaunchKernelGGL(hetrd_correct_kernel<R>, dim3(grblocks_of(m)), dim3(GT), 0, s, n, i, j0, A, lda, wk,
                       symv_lower_tpw(m), i > j0 ? int(gblocks_of(m)) : 0);
}

#define SLATE_INST_HETRD(R)                                                                                  \
    template void symv_lower<R>(int64_t, const R*, int64_t, const R*, R*, R*, hipStream_t);                \
    template void hetrd_column<R>(int64_t, int64_t, int64_t, bool, R*, int64_t, HetrdWork<R> const&, hipStream_t); \
    template void hetrd_larfg<R>(int64_t, int64_t, R*, int64_t, HetrdWork<R> const&, hipStream_t);         \
    template void hetrd_symv<R>(int64_t, int64_t, int64_t, const R*, int64_t, HetrdWork<R> const&, hipStream_t); \
    template void hetrd_correct<R>(int64_t, int64_t, int64_t, const R*, int64_t, HetrdWork<R> const&, hipStream_t);

SLATE_INST_HETRD(float)
SLATE_INST_HETRD(double)

}  // namespace dev
}  // namespace slate_amd
