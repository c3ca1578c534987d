// Device helpers shared by the kernels of the one-stage reductions (hetrd.hip,
// gebrd.hip, geqp3.hip, larfg_vec.hip): the fixed-order block reductions,
// larfg from a sum of squares, the 64 x 16 tile scheme of the product A^T x
// with its column-partial reduction, and the small dots with the panel that
// ride in the product grids.
//
// The tile scheme: the block is cut into tiles of 64 rows x 16 columns.  A
// lane owns one row of a tile, so a wave reads 64 consecutive elements of a
// column: coalesced whatever the alignment of the block's base.  A workgroup
// takes one block column and 4 x tpw row tiles, its waves taking different
// tiles; the 16 column partials stay in registers over the wave's tiles and
// are reduced once through LDS.  Loads outside the block are masked.
//
// The small dots: the workgroups of a product grid with blockIdx.y >= nJ take
// 256 rows each of the products of the panel's columns with the current
// vector (panel_dots), their partials go to pdots, and every workgroup of the
// finishing kernel sums them again in the same order (gather_pdots).
#pragma once
#include "device_common.hh"
#include "kernels.hh"

namespace slate_amd {
namespace dev {

namespace {

constexpr int GT = 256;    // threads of every kernel here
constexpr int TR = 64;     // tile rows = lanes
constexpr int TC = 16;     // tile columns
constexpr int GR = 64;     // rows (columns) per workgroup of the row kernels: a lane owns one, the 4 waves split the sums
constexpr int KP = kReducePanel;   // columns of a panel: the LDS rows of the panel and the slots of pdots

// block sum, the same bits in every thread; all threads of the block call it
template <typename R>
__device__ inline R gb_block_sum(R v, R* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// sum over the 4 waves of each lane's value, the same bits in all of them
template <typename R>
__device__ inline R gb_waves_sum(R v, R (*red)[GR]) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    __syncthreads();
    red[g][lane] = v;
    __syncthreads();
    return (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// sum of cnt workgroup partials, the same bits in every thread of every workgroup
template <typename R>
__device__ inline R gb_partial_sum(const R* p, int cnt, R* sh) {
    R s = R(0);
    for (int q = threadIdx.x; q < cnt; q += GT) s += p[q];
    return gb_block_sum<R>(s, sh);
}

// larfg from alpha and the sum of squares of the tail
template <typename R>
__device__ inline void gb_larfg(R alpha, R ss, R& beta, R& tau, R& scale) {
    beta = alpha; tau = R(0); scale = R(0);
    if (ss != R(0)) {
        const R nrm = sqrt(alpha * alpha + ss);
        beta = alpha >= R(0) ? -nrm : nrm;
        tau = (beta - alpha) / beta;
        scale = R(1) / (alpha - beta);
    }
}

// the TC column partials that each lane holds -> out[0:ncol]: lanes -> LDS (cbuf: 4 TC rows of 65),
// one thread per (wave, column) sums the 64 lanes in order into slot 64 of its row (not read by
// anyone before the next barrier), then the 4 waves
template <typename R>
__device__ inline void gb_colpart_reduce(const R (&cacc)[TC], int ncol, R* out, R* cbuf) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int c = 0; c < TC; ++c) cbuf[(w * TC + c) * 65 + lane] = cacc[c];
    __syncthreads();
    if (threadIdx.x < 4 * TC) {
        const R* q = cbuf + threadIdx.x * 65;
        R v = R(0);
        for (int l = 0; l < 64; ++l) v += q[l];
        cbuf[threadIdx.x * 65 + 64] = v;
    }
    __syncthreads();
    if (int(threadIdx.x) < ncol) {
        const int c = threadIdx.x;
        out[c] = (cbuf[(0 * TC + c) * 65 + 64] + cbuf[(1 * TC + c) * 65 + 64]) +
                 (cbuf[(2 * TC + c) * 65 + 64] + cbuf[(3 * TC + c) * 65 + 64]);
    }
}

// one workgroup of A^T x over the mr x nc block at A: block column J, chunk k.
// colpart[k * nc + j] = sum over the chunk's rows of A(r, j) x(r)
template <typename R>
__device__ inline void gemv_t_tiles(int64_t mr, int64_t nc, const R* A, int64_t lda, const R* x, R* colpart, int tpw,
                                    int64_t k, int64_t J, R* cbuf) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = J * TC;
    const int ncol = int(min(int64_t(TC), nc - c0));
    const int64_t nRT = (mr + TR - 1) / TR;
    const int64_t tbase = k * (4 * tpw);
    R cacc[TC];
    #pragma unroll
    for (int c = 0; c < TC; ++c) cacc[c] = R(0);
    for (int s = 0; s < tpw; ++s) {
        const int64_t t = tbase + w + 4 * s;
        if (t >= nRT) break;    // uniform over the wave
        const int64_t r = t * TR + lane;
        const bool inb = r < mr;
        const R* ap = A + r + c0 * lda;
        const R xr = inb ? x[r] : R(0);
        #pragma unroll
        for (int c = 0; c < TC; ++c) {
            // a masked lane loads x[0] instead (a valid address) and drops it: no branch per load
            const bool ok = inb && c < ncol;
            const R ld = *(ok ? ap + c * lda : x);
            cacc[c] += ok ? ld * xr : R(0);
        }
    }
    gb_colpart_reduce<R>(cacc, ncol, colpart + k * nc + c0, cbuf);
}

// workgroup q of the small dots: entries r0 .. r0 + 255 (below rend) of x against the nk columns of
// A (and, with Two, of B), one wave per column, rows indexed as x is:
// out[k] = sum_r A(r, k) x(r), out[KP + k] = sum_r B(r, k) x(r)
template <typename R, bool Two>
__device__ inline void panel_dots(int64_t r0, int64_t rend, const R* x, int nk, const R* A, int64_t lda, const R* B,
                                  int64_t ldb, R* out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    R xr[4];
    #pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int64_t r = r0 + lane + 64 * s;
        xr[s] = r < rend ? x[r] : R(0);
    }
    for (int k = w; k < nk; k += 4) {
        R sa = R(0), sb = R(0);
        #pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t r = r0 + lane + 64 * s;
            if (r < rend) {
                sa += A[r + int64_t(k) * lda] * xr[s];
                if constexpr (Two) sb += B[r + int64_t(k) * ldb] * xr[s];
            }
        }
        sa = wave_sum(sa);
        if constexpr (Two) sb = wave_sum(sb);
        if (lane == 0) {
            out[k] = sa;
            if constexpr (Two) out[KP + k] = sb;
        }
    }
}

// t[x] = sum over the ndots workgroups of pdots[q * stride + x] in order, for the first n0 of the
// first KP slots and the first n1 of the second (stride = KP or 2 KP); the caller's barrier follows
template <typename R>
__device__ inline void gather_pdots(const R* pdots, int ndots, int stride, int n0, int n1, R* t) {
    const int x = threadIdx.x;
    if (x < stride && (x & 63) < (x < KP ? n0 : n1)) {
        R s = R(0);
        for (int q = 0; q < ndots; ++q) s += pdots[int64_t(q) * stride + x];
        t[x] = s;
    }
}

inline unsigned gblocks_of(int64_t rows) { return unsigned((rows + GT - 1) / GT); }
inline unsigned grblocks_of(int64_t rows) { return unsigned((rows + GR - 1) / GR); }

// grid of a product with the small dots riding along: nk chunks x nJ block columns, then enough
// rows of nk workgroups for the ndots workgroups of panel_dots (q = (blockIdx.y - nJ) nk + blockIdx.x)
inline dim3 product_grid(int64_t nk, int64_t nJ, int64_t ndots) {
    return dim3(unsigned(nk), unsigned(nJ + (ndots + nk - 1) / nk));
}

}  // namespace

}  // namespace dev
}  // namespace slate_amd
