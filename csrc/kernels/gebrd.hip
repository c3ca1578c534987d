// Device side of the one-stage bidiagonal reduction (src/gebrd.cc; LAPACK's
// gebrd / labrd, written from the math), real types, m >= n, upper bidiagonal.
//
// Column i of a panel that starts at j0 (c = i - j0; U = A(:, j0:i) the left
// reflectors, V = A(j0:i, :) the right ones, X m x 64 and Y n x 64 the
// workspaces) takes seven launches, every dependency between workgroups being
// a kernel boundary (no flags, no waiting, no atomics):
//   1 gebrd_column   A(i:m, i) -= U Y(i,:)^T + X V(:, i), alpha and the
//                    per-workgroup sums of squares below it
//   2 gebrd_larfg_u  beta, tauq from those sums (d_i = beta); u scaled in
//                    place, unit entry stored, u copied to a contiguous vector
//                    (larfg_vec.hip, as 5)
//   3 gebrd_pass1    partials of A(i:m, i+1:n)^T u, and in the same grid the
//                    partials of U^T u and X^T u
//   4 gebrd_finish_y partials summed in a fixed order, y = tauq (A^T u -
//                    Y (U^T u) - V^T (X^T u)); row i of A updated with it:
//                    A(i, i+1:n) -= U(i,:) Y^T + X(i,:) V; sums of squares
//   5 gebrd_larfg_v  beta, taup (e_i = beta); v scaled, unit entry stored
//   6 gebrd_pass2    partials of A(i+1:m, i+1:n) v, and in the same grid the
//                    partials of Y^T v and V v
//   7 gebrd_finish_x x = taup (A v - U (Y^T v) - X (V v))
// The last column of the matrix takes the first two only.  Every reduction
// has two levels: partials go to a workspace, and every workgroup of the next
// kernel sums them again in the same order, so all workgroups see the same
// bits and two runs give identical results.
//
// The two products use the 64 x 16 tiles that reduce_tiles.hh describes; the
// block's base is only element-aligned and moves every column.  Pass 1 (A^T u)
// is gemv_t_tiles of that header, as are the small dots and their gather;
// pass 2 (A v, gemv_n_tiles below) writes each tile's row sums per block
// column.  Loads outside the block are masked: nothing outside it is read.
#include "device_common.hh"
#include "reduce_tiles.hh"
#include "kernels.hh"

#include <algorithm>

namespace slate_amd {
namespace dev {

namespace {

// GT, TR, TC, GR, KP, the gb_* reductions, gemv_t_tiles (A^T x), panel_dots and gather_pdots: reduce_tiles.hh

// one workgroup of A x over the mr x nc block at A: block column J, chunk k.
// rowpart[J * mr + r] = sum over the block column of A(r, j) x(j).  The wave's
// tiles go two at a time, all 32 loads ahead of the two stores (rowpart does
// not alias A: __restrict__), so the next tile's loads do not wait for a store.
template <typename R>
__device__ inline void gemv_n_tiles(int64_t mr, int64_t nc, const R* __restrict__ A, int64_t lda,
                                    const R* __restrict__ x, R* __restrict__ rowpart, int tpw, int64_t k, int64_t J) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = J * TC;
    const int ncol = int(min(int64_t(TC), nc - c0));
    const int64_t nRT = (mr + TR - 1) / TR;
    const int64_t tbase = k * (4 * tpw);
    R xc[TC];
    #pragma unroll
    for (int c = 0; c < TC; ++c) xc[c] = c < ncol ? x[c0 + c] : R(0);
    for (int s = 0; s < tpw; s += 2) {
        const int64_t t0 = tbase + w + 4 * s, t1 = t0 + 4;
        if (t0 >= nRT) break;    // uniform over the wave
        const int64_t r0 = t0 * TR + lane, r1 = t1 * TR + lane;
        const bool in0 = r0 < mr, in1 = s + 1 < tpw && r1 < mr;
        const R* ap0 = A + r0 + c0 * lda;
        const R* ap1 = A + r1 + c0 * lda;
        R a0[TC], a1[TC];
        #pragma unroll
        for (int c = 0; c < TC; ++c) {
            // a masked lane loads x[0] instead (a valid address) and drops it: no branch per load
            a0[c] = *(in0 && c < ncol ? ap0 + c * lda : x);
            a1[c] = *(in1 && c < ncol ? ap1 + c * lda : x);
        }
        R s0 = R(0), s1 = R(0);
        #pragma unroll
        for (int c = 0; c < TC; ++c) {
            s0 += in0 && c < ncol ? a0[c] * xc[c] : R(0);
            s1 += in1 && c < ncol ? a1[c] * xc[c] : R(0);
        }
        if (in0) rowpart[J * mr + r0] = s0;
        if (in1) rowpart[J * mr + r1] = s1;
    }
}

template <typename R>
__global__ __launch_bounds__(GT) void gemv_t_block_kernel(int64_t mr, int64_t nc, const R* A, int64_t lda, const R* x,
                                                          R* colpart, int tpw) {
    __shared__ R cbuf[4 * TC * 65];
    gemv_t_tiles<R>(mr, nc, A, lda, x, colpart, tpw, blockIdx.x, blockIdx.y, cbuf);
}

template <typename R>
__global__ __launch_bounds__(GT) void gemv_n_block_kernel(int64_t mr, int64_t nc, const R* A, int64_t lda, const R* x,
                                                          R* rowpart, int tpw) {
    gemv_n_tiles<R>(mr, nc, A, lda, x, rowpart, tpw, blockIdx.x, blockIdx.y);
}

// y_j = sum over the nk chunks of colpart, lane = column, the 4 waves split the chunks
template <typename R>
__global__ __launch_bounds__(GT) void gemv_t_reduce_kernel(int64_t nc, int nk, const R* colpart, R* y) {
    __shared__ R red[4][GR];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t j = int64_t(blockIdx.x) * GR + lane;
    R s = R(0);
    if (j < nc)
        for (int k = g; k < nk; k += 4) s += colpart[int64_t(k) * nc + j];
    s = gb_waves_sum<R>(s, red);
    if (j < nc && g == 0) y[j] = s;
}

template <typename R>
__global__ __launch_bounds__(GT) void gemv_n_reduce_kernel(int64_t mr, int nJ, const R* rowpart, R* y) {
    __shared__ R red[4][GR];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t r = int64_t(blockIdx.x) * GR + lane;
    R s = R(0);
    if (r < mr) {
        #pragma unroll 16
        for (int J = g; J < nJ; J += 4) s += rowpart[int64_t(J) * mr + r];   // 16 loads in flight, summed in order
    }
    s = gb_waves_sum<R>(s, red);
    if (r < mr && g == 0) y[r] = s;
}

//------------------------------------------------------------------------------
// 1: rows r >= i.  A(r, i) -= sum_k U(r, k) Y(i, k) + X(r, k) V(k, i)
template <typename R>
__global__ __launch_bounds__(GT) void gebrd_column_kernel(int64_t m, int64_t i, int64_t j0, R* A, int64_t lda,
                                                          GebrdWork<R> wk) {
    __shared__ R sh[4];
    __shared__ R Yi[KP], Vi[KP];
    __shared__ R red[4][GR];
    const int c = int(i - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t r = i + int64_t(blockIdx.x) * GR + lane;
    const bool inb = r < m;
    if (int(threadIdx.x) < c) {
        const int k = threadIdx.x;
        Yi[k] = wk.Y[i + int64_t(k) * wk.ldy];
        Vi[k] = A[(j0 + k) + i * lda];
    }
    __syncthreads();
    R s = R(0);
    if (inb) {
        #pragma unroll 4
        for (int k = g; k < c; k += 4) s += A[r + (j0 + k) * lda] * Yi[k] + wk.X[r + int64_t(k) * wk.ldx] * Vi[k];
    }
    s = gb_waves_sum<R>(s, red);
    R a = R(0);
    if (inb && g == 0) {
        a = A[r + i * lda] - s;
        A[r + i * lda] = a;
        if (r == i) wk.scal[0] = a;
    }
    const R ss = gb_block_sum<R>(g == 0 && inb && r > i ? a * a : R(0), sh);
    if (threadIdx.x == 0) wk.ssq[blockIdx.x] = ss;
}

// 3: partials of A(i:m, i+1:n)^T u, and (blockIdx.y >= nJ) the partials of
// U^T u and X^T u over 256 rows each, one wave per column
template <typename R>
__global__ __launch_bounds__(GT) void gebrd_pass1_kernel(int64_t m, int64_t n, int64_t i, int64_t j0, const R* A,
                                                         int64_t lda, GebrdWork<R> wk, int tpw, int nJ, int ndots) {
    __shared__ R cbuf[4 * TC * 65];
    if (int(blockIdx.y) < nJ) {
        gemv_t_tiles<R>(m - i, n - i - 1, A + i + (i + 1) * lda, lda, wk.u + i, wk.colpart, tpw, blockIdx.x, blockIdx.y,
                        cbuf);
        return;
    }
    const int64_t q = int64_t(blockIdx.y - nJ) * gridDim.x + blockIdx.x;
    if (q >= ndots) return;
    panel_dots<R, true>(i + q * GT, m, wk.u, int(i - j0), A + j0 * lda, lda, wk.X, wk.ldx, wk.pdots + q * (2 * KP));
}

// 4: columns j > i, lane = column.  y_j finished and stored in Y(j, c), row i of A updated
template <typename R>
__global__ __launch_bounds__(GT) void gebrd_finish_y_kernel(int64_t m, int64_t n, int64_t i, int64_t j0, R* A,
                                                            int64_t lda, GebrdWork<R> wk, int nk, int ndots) {
    __shared__ R sh[4];
    __shared__ R t12[2 * KP];   // U^T u | X^T u
    __shared__ R Ui[KP], Xi[KP];
    __shared__ R red[4][GR];
    const int c = int(i - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    gather_pdots<R>(wk.pdots, ndots, 2 * KP, c, c, t12);
    if (threadIdx.x >= 128 && threadIdx.x < 192 && lane < c) Ui[lane] = A[i + (j0 + lane) * lda];
    if (threadIdx.x >= 192 && lane < c) Xi[lane] = wk.X[i + int64_t(lane) * wk.ldx];
    __syncthreads();
    const int64_t nc = n - i - 1;
    const int64_t jl = int64_t(blockIdx.x) * GR + lane, j = i + 1 + jl;
    const bool inb = j < n;
    // wave g's share of the three sums of y_j and of the two of the row update
    R ys = R(0), rs = R(0);
    if (inb) {
        for (int k = g; k < nk; k += 4) ys += wk.colpart[int64_t(k) * nc + jl];
        #pragma unroll 4
        for (int k = g; k < c; k += 4) {
            const R yk = wk.Y[j + int64_t(k) * wk.ldy], vk = A[(j0 + k) + j * lda];
            ys -= yk * t12[k] + vk * t12[KP + k];
            rs += yk * Ui[k] + vk * Xi[k];
        }
    }
    ys = gb_waves_sum<R>(ys, red);
    rs = gb_waves_sum<R>(rs, red);
    R a = R(0);
    if (inb && g == 0) {
        const R y = wk.tauq[i] * ys;
        wk.Y[j + int64_t(c) * wk.ldy] = y;
        a = A[i + j * lda] - rs - y;    // U(i, c) = 1
        A[i + j * lda] = a;
        if (j == i + 1) wk.scal[1] = a;
    }
    const R ss = gb_block_sum<R>(g == 0 && inb && j > i + 1 ? a * a : R(0), sh);
    if (threadIdx.x == 0) wk.ssq2[blockIdx.x] = ss;
}

// 6: partials of A(i+1:m, i+1:n) v, and (blockIdx.y >= nJ) the partials of
// Y(i+1:n, 0:c+1)^T v (one wave per column) and of V(0:c, i+1:n) v (lane =
// row of V, a wave takes 64 columns) over 256 columns each
template <typename R>
__global__ __launch_bounds__(GT) void gebrd_pass2_kernel(int64_t m, int64_t n, int64_t i, int64_t j0, const R* A,
                                                         int64_t lda, GebrdWork<R> wk, int tpw, int nJ, int ndots) {
    __shared__ R red[4][GR];
    if (int(blockIdx.y) < nJ) {
        gemv_n_tiles<R>(m - i - 1, n - i - 1, A + (i + 1) + (i + 1) * lda, lda, wk.v + i + 1, wk.rowpart, tpw,
                        blockIdx.x, blockIdx.y);
        return;
    }
    const int64_t q = int64_t(blockIdx.y - nJ) * gridDim.x + blockIdx.x;
    if (q >= ndots) return;
    const int c = int(i - j0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = i + 1 + q * GT;
    panel_dots<R, false>(c0, n, wk.v, c + 1, wk.Y, wk.ldy, nullptr, 0, wk.pdots + q * (2 * KP));
    // V v: lane = k, wave w takes columns c0 + 64 w .. + 63
    R sv = R(0);
    if (lane < c) {
        const int64_t jb = c0 + 64 * w, je = min(n, jb + 64);
        for (int64_t j = jb; j < je; ++j) sv += A[(j0 + lane) + j * lda] * wk.v[j];
    }
    sv = gb_waves_sum<R>(sv, red);
    if (w == 0 && lane < c) wk.pdots[q * (2 * KP) + KP + lane] = sv;
}

// 7: rows r > i.  x_r finished and stored in X(r, c)
template <typename R>
__global__ __launch_bounds__(GT) void gebrd_finish_x_kernel(int64_t m, int64_t n, int64_t i, int64_t j0, const R* A,
                                                            int64_t lda, GebrdWork<R> wk, int nJ, int ndots) {
    __shared__ R t34[2 * KP];   // Y^T v (c + 1) | V v (c)
    __shared__ R red[4][GR];
    const int c = int(i - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    gather_pdots<R>(wk.pdots, ndots, 2 * KP, c + 1, c, t34);
    __syncthreads();
    const int64_t mr = m - i - 1;
    const int64_t rl = int64_t(blockIdx.x) * GR + lane, r = i + 1 + rl;
    const bool inb = r < m;
    R xs = R(0);
    if (inb) {
        #pragma unroll 16
        for (int J = g; J < nJ; J += 4) xs += wk.rowpart[int64_t(J) * mr + rl];
        #pragma unroll 4
        for (int k = g; k <= c; k += 4) {
            xs -= A[r + (j0 + k) * lda] * t34[k];
            if (k < c) xs -= wk.X[r + int64_t(k) * wk.ldx] * t34[KP + k];
        }
    }
    xs = gb_waves_sum<R>(xs, red);
    if (inb && g == 0) wk.X[r + int64_t(c) * wk.ldx] = wk.taup[i] * xs;
}

// explicit transposed row block of the right reflectors of a panel: out (nv x
// kb, unit lower trapezoid), out(j, k) = A(j0 + k, j0 + 1 + j) below the diagonal
template <typename R>
__global__ __launch_bounds__(GT) void gebrd_form_vt_kernel(int64_t nv, int kb, const R* Arow, int64_t lda, R* out,
                                                           int64_t ldo) {
    // Arow = A + j0 + (j0 + 1) lda; thread (k fastest) reads down a column of A
    const int64_t idx = int64_t(blockIdx.x) * GT + threadIdx.x;
    const int64_t j = idx / kb;
    const int k = int(idx % kb);
    if (j >= nv) return;
    out[j + int64_t(k) * ldo] = j < k ? R(0) : (j == k ? R(1) : Arow[k + j * lda]);
}

}  // namespace

int gemv_block_tpw(int64_t mr, int64_t nc) {
    const int64_t nRT = (mr + TR - 1) / TR, nJ = (nc + TC - 1) / TC;
    return int(std::max<int64_t>(1, std::min<int64_t>(8, nRT * nJ / (4 * 512))));
}
int64_t gemv_block_chunks(int64_t mr, int tpw) {
    return std::max<int64_t>(1, ((mr + TR - 1) / TR + 4 * tpw - 1) / (4 * tpw));
}
int64_t gemv_t_block_workspace(int64_t mr, int64_t nc) {
    return std::max<int64_t>(1, gemv_block_chunks(mr, gemv_block_tpw(mr, nc)) * nc);
}
int64_t gemv_n_block_workspace(int64_t mr, int64_t nc) {
    return std::max<int64_t>(1, ((nc + TC - 1) / TC) * mr);
}

template <typename R>
void gemv_t_block(int64_t mr, int64_t nc, const R* A, int64_t lda, const R* x, R* y, R* work, hipStream_t s) {
    if (mr <= 0 || nc <= 0) return;
    const int tpw = gemv_block_tpw(mr, nc);
    const int64_t nJ = (nc + TC - 1) / TC, nk = gemv_block_chunks(mr, tpw);
    hipLaunchKernelGGL(gemv_t_block_kernel<R>, dim3(unsigned(nk), unsigned(nJ)), dim3(GT), 0, s, mr, nc, A, lda, x,
                       work, tpw);
    hipLaunchKernelGGL(gemv_t_reduce_kernel<R>, dim3(grblocks_of(nc)), dim3(GT), 0, s, nc, int(nk), work, y);
}

template <typename R>
void gemv_n_block(int64_t mr, int64_t nc, const R* A, int64_t lda, const R* x, R* y, R* work, hipStream_t s) {
    if (mr <= 0 || nc <= 0) return;
    const int tpw = gemv_block_tpw(mr, nc);
    const int64_t nJ = (nc + TC - 1) / TC, nk = gemv_block_chunks(mr, tpw);
    hipLaunchKernelGGL(gemv_n_block_kernel<R>, dim3(unsigned(nk), unsigned(nJ)), dim3(GT), 0, s, mr, nc, A, lda, x,
                       work, tpw);
    hipLaunchKernelGGL(gemv_n_reduce_kernel<R>, dim3(grblocks_of(mr)), dim3(GT), 0, s, mr, int(nJ), work, y);
}

template <typename R>
void gebrd_column(int64_t m, int64_t i, int64_t j0, R* A, int64_t lda, GebrdWork<R> const& wk, hipStream_t s) {
    hipLaunchKernelGGL(gebrd_column_kernel<R>, dim3(grblocks_of(m - i)), dim3(GT), 0, s, m, i, j0, A, lda, wk);
}
template <typename R>
void gebrd_larfg_u(int64_t m, int64_t i, R* A, int64_t lda, GebrdWork<R> const& wk, hipStream_t s) {
    larfg_vec<R>(m - i, A + i + i * lda, 1, wk.scal, wk.ssq, int(grblocks_of(m - i)), wk.tauq + i, wk.d + i, wk.u + i,
                 false, s);
}
template <typename R>
void gebrd_pass1(int64_t m, int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda, GebrdWork<R> const& wk,
                 hipStream_t s) {
    const int64_t mr = m - i, nc = n - i - 1;
    const int tpw = gemv_block_tpw(mr, nc);
    const int64_t nJ = (nc + TC - 1) / TC, nk = gemv_block_chunks(mr, tpw);
    const int64_t ndots = i > j0 ? gblocks_of(mr) : 0;
    hipLaunchKernelGGL(gebrd_pass1_kernel<R>, product_grid(nk, nJ, ndots), dim3(GT), 0, s, m, n, i, j0, A, lda, wk, tpw,
                       int(nJ), int(ndots));
}
template <typename R>
void gebrd_finish_y(int64_t m, int64_t n, int64_t i, int64_t j0, R* A, int64_t lda, GebrdWork<R> const& wk,
                    hipStream_t s) {
    const int64_t mr = m - i, nc = n - i - 1;
    const int64_t nk = gemv_block_chunks(mr, gemv_block_tpw(mr, nc));
    hipLaunchKernelGGL(gebrd_finish_y_kernel<R>, dim3(grblocks_of(nc)), dim3(GT), 0, s, m, n, i, j0, A, lda, wk,
                       int(nk), i > j0 ? int(gblocks_of(mr)) : 0);
}
template <typename R>
void gebrd_larfg_v(int64_t n, int64_t i, R* A, int64_t lda, GebrdWork<R> const& wk, hipStream_t s) {
    const int64_t nc = n - i - 1;
    larfg_vec<R>(nc, A + i + (i + 1) * lda, lda, wk.scal + 1, wk.ssq2, int(grblocks_of(nc)), wk.taup + i, wk.e + i,
                 wk.v + i + 1, false, s);
}
template <typename R>
void gebrd_pass2(int64_t m, int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda, GebrdWork<R> const& wk,
                 hipStream_t s) {
    const int64_t mr = m - i - 1, nc = n - i - 1;
    if (mr <= 0 || nc <= 0) return;
    const int64_t ndots = gblocks_of(nc);    // Y^T v has the new column of Y even when c = 0
    const int tpw = gemv_block_tpw(mr, nc);
    const int64_t nJ = (nc + TC - 1) / TC, nk = gemv_block_chunks(mr, tpw);
    hipLaunchKernelGGL(gebrd_pass2_kernel<R>, product_grid(nk, nJ, ndots), dim3(GT), 0, s, m, n, i, j0, A, lda, wk, tpw,
                       int(nJ), int(ndots));
}
template <typename R>
void gebrd_finish_x(int64_t m, int64_t n, int64_t i, int64_t j0, const R* A, int64_t lda, GebrdWork<R> const& wk,
                    hipStream_t s) {
    const int64_t mr = m - i - 1, nc = n - i - 1;
    if (mr <= 0) return;
    hipLaunchKernelGGL(gebrd_finish_x_kernel<R>, dim3(grblocks_of(mr)), dim3(GT), 0, s, m, n, i, j0, A, lda, wk,
                       int((nc + TC - 1) / TC), int(gblocks_of(nc)));
}
template <typename R>
void gebrd_form_vt(int64_t nv, int kb, const R* Arow, int64_t lda, R* out, int64_t ldo, hipStream_t s) {
    if (nv <= 0 || kb <= 0) return;
    hipLaunchKernelGGL(gebrd_form_vt_kernel<R>, dim3(gblocks_of(nv * kb)), dim3(GT), 0, s, nv, kb, Arow, lda, out, ldo);
}

#define SLATE_INST_GEBRD(R)                                                                                       \
    template void gemv_t_block<R>(int64_t, int64_t, const R*, int64_t, const R*, R*, R*, hipStream_t);            \
    template void gemv_n_block<R>(int64_t, int64_t, const R*, int64_t, const R*, R*, R*, hipStream_t);            \
    template void gebrd_column<R>(int64_t, int64_t, int64_t, R*, int64_t, GebrdWork<R> const&, hipStream_t);      \
    template void gebrd_larfg_u<R>(int64_t, int64_t, R*, int64_t, GebrdWork<R> const&, hipStream_t);              \
    template void gebrd_pass1<R>(int64_t, int64_t, int64_t, int64_t, const R*, int64_t, GebrdWork<R> const&,      \
                                 hipStream_t);                                                                    \
    template void gebrd_finish_y<R>(int64_t, int64_t, int64_t, int64_t, R*, int64_t, GebrdWork<R> const&,         \
                                    hipStream_t);                                                                 \
    template void gebrd_larfg_v<R>(int64_t, int64_t, R*, int64_t, GebrdWork<R> const&, hipStream_t);              \
    template void gebrd_pass2<R>(int64_t, int64_t, int64_t, int64_t, const R*, int64_t, GebrdWork<R> const&,      \
                                 hipStream_t);                                                                    \
    template void gebrd_finish_x<R>(int64_t, int64_t, int64_t, int64_t, const R*, int64_t, GebrdWork<R> const&,   \
                                    hipStream_t);                                                                 \
    template void gebrd_form_vt<R>(int64_t, int, const R*, int64_t, R*, int64_t, hipStream_t);

SLATE_INST_GEBRD(float)
SLATE_INST_GEBRD(double)

}  // namespace dev
}  // namespace slate_amd
