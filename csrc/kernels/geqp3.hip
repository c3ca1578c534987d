// Device side of the QR factorization with column pivoting (src/geqp3.cc;
// LAPACK's geqp3 / laqps, written from the math), real types, any m and n.
//
// Column j of a panel that starts at j0 (jj = j - j0; V = A(:, j0:j) the
// reflectors of the panel, F n x 64 the workspace with A22 -= V F^T pending,
// vn1 / vn2 the partial and the reference column norms) takes seven launches,
// every dependency between workgroups being a kernel boundary (no flags, no
// waiting, no atomics) and nothing going to the host:
//   1 geqp3_pivot     p = argmax vn1[j:n], the smallest index among equal
//                     maxima: one workgroup, a wave-level argmax
//   2 geqp3_swap      columns j and p of A over all m rows, rows j and p of F,
//                     vn1, vn2 and jpvt
//   3 geqp3_column    A(j:m, j) -= V(j:m, :) F(j, 0:jj)^T, alpha and the
//                     per-workgroup sums of squares below it
//   4 geqp3_larfg     beta, tau from those sums (R_jj = beta stays in A); v
//                     scaled in place and copied, with its unit entry, to a
//                     contiguous vector (larfg_vec.hip)
//   5 geqp3_product   partials of A(j:m, j+1:n)^T v, and in the same grid the
//                     partials of V(j:m, :)^T v
//   6 geqp3_finish    partials summed in a fixed order, F(c, jj) = tau (A^T v -
//                     F (V^T v)); row j of A updated: A(j, c) -= V(j, :) F(c, :)^T;
//                     LAPACK's norm downdate of vn1[c], or the column flagged
//                     when cancellation makes the downdated norm untrustworthy
//   7 geqp3_recompute a workgroup per column c > j leaves at once unless its
//                     column is flagged; then it forms the updated column
//                     A(j+1:m, c) - V(j+1:m, :) F(c, :)^T in a fixed order,
//                     stores it and clears F(c, :) (the update of this column
//                     is no longer pending), sets vn1[c] = vn2[c] to its norm
//                     and counts the recompute in the slot of its column
// The last column of the matrix takes steps 3 and 4 only.  Every reduction has
// two levels and a fixed order, so two runs give identical results.  The
// product uses the 64 x 16 tiles of reduce_tiles.hh, which also has the small
// dots and their gather: one read of the trailing block per column.  Loads
// outside the matrix are masked.
#include "device_common.hh"
#include "reduce_tiles.hh"
#include "kernels.hh"

#include <algorithm>

namespace slate_amd {
namespace dev {

namespace {

// column norms: one workgroup per column, strided partial sums, then the block sum
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_norms_kernel(int64_t m, const R* A, int64_t lda, Geqp3Work<R> wk) {
    __shared__ R sh[4];
    const int64_t c = blockIdx.x;
    const R* a = A + c * lda;
    R s = R(0);
    for (int64_t r = threadIdx.x; r < m; r += GT) s += a[r] * a[r];
    s = gb_block_sum<R>(s, sh);
    if (threadIdx.x == 0) {
        const R nrm = sqrt(s);
        wk.vn1[c] = nrm;
        wk.vn2[c] = nrm;
        wk.jpvt[c] = c;
        wk.recomputes[c] = 0;
        wk.flag[c] = 0;
    }
}

// (value, index) a before b: the larger value, the smaller index among equal ones
template <typename R>
__device__ inline bool gq_before(R av, int ai, R bv, int bi) { return av > bv || (av == bv && ai < bi); }

// 1: one workgroup.  A NaN never wins; with nothing but NaNs the pivot is j
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_pivot_kernel(int64_t n, int64_t j, Geqp3Work<R> wk) {
    __shared__ R bvs[4];
    __shared__ int bis[4];
    R bv = R(-1);
    int bi = int(n);
    for (int64_t c = j + threadIdx.x; c < n; c += GT) {
        const R x = wk.vn1[c];
        if (x > bv) { bv = x; bi = int(c); }
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const R ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (gq_before<R>(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bvs[threadIdx.x >> 6] = bv; bis[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (gq_before<R>(bvs[w], bis[w], bv, bi)) { bv = bvs[w]; bi = bis[w]; }
        wk.piv[0] = bi < n ? int64_t(bi) : j;
    }
}

// 2: all m rows of columns j and p; workgroup 0 also rows j and p of F (the jj columns written so
// far), vn1, vn2 and jpvt
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_swap_kernel(int64_t m, int64_t j, int64_t j0, R* A, int64_t lda,
                                                        Geqp3Work<R> wk) {
    const int64_t p = wk.piv[0];
    if (p == j) return;
    const int64_t r = int64_t(blockIdx.x) * GT + threadIdx.x;
    if (r < m) {
        const R x = A[r + j * lda];
        A[r + j * lda] = A[r + p * lda];
        A[r + p * lda] = x;
    }
    if (blockIdx.x != 0) return;
    const int jj = int(j - j0);
    if (int(threadIdx.x) < jj) {
        const int64_t k = threadIdx.x;
        const R x = wk.F[j + k * wk.ldf];
        wk.F[j + k * wk.ldf] = wk.F[p + k * wk.ldf];
        wk.F[p + k * wk.ldf] = x;
    }
    if (threadIdx.x == GT - 1) {
        const R x1 = wk.vn1[j], x2 = wk.vn2[j];
        wk.vn1[j] = wk.vn1[p]; wk.vn1[p] = x1;
        wk.vn2[j] = wk.vn2[p]; wk.vn2[p] = x2;
        const int64_t t = wk.jpvt[j];
        wk.jpvt[j] = wk.jpvt[p]; wk.jpvt[p] = t;
    }
}

// 3: rows r >= j.  A(r, j) -= sum_k V(r, k) F(j, k)
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_column_kernel(int64_t m, int64_t j, int64_t j0, R* A, int64_t lda,
                                                          Geqp3Work<R> wk) {
    __shared__ R sh[4];
    __shared__ R Fj[KP];
    __shared__ R red[4][GR];
    const int jj = int(j - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t r = j + int64_t(blockIdx.x) * GR + lane;
    const bool inb = r < m;
    if (int(threadIdx.x) < jj) Fj[threadIdx.x] = wk.F[j + int64_t(threadIdx.x) * wk.ldf];
    __syncthreads();
    R s = R(0);
    if (inb) {
        #pragma unroll 4
        for (int k = g; k < jj; k += 4) s += A[r + (j0 + k) * lda] * Fj[k];
    }
    s = gb_waves_sum<R>(s, red);
    R a = R(0);
    if (inb && g == 0) {
        a = A[r + j * lda] - s;
        A[r + j * lda] = a;
        if (r == j) wk.scal[0] = a;
    }
    const R ss = gb_block_sum<R>(g == 0 && inb && r > j ? a * a : R(0), sh);
    if (threadIdx.x == 0) wk.ssq[blockIdx.x] = ss;
}

// 5: partials of A(j:m, j+1:n)^T v, and (blockIdx.y >= nJ) the partials of
// V(j:m, 0:jj)^T v over 256 rows each, one wave per column
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_product_kernel(int64_t m, int64_t n, int64_t j, int64_t j0, const R* A,
                                                           int64_t lda, Geqp3Work<R> wk, int tpw, int nJ, int ndots) {
    __shared__ R cbuf[4 * TC * 65];
    if (int(blockIdx.y) < nJ) {
        gemv_t_tiles<R>(m - j, n - j - 1, A + j + (j + 1) * lda, lda, wk.v + j, wk.colpart, tpw, blockIdx.x, blockIdx.y,
                        cbuf);
        return;
    }
    const int64_t q = int64_t(blockIdx.y - nJ) * gridDim.x + blockIdx.x;
    if (q >= ndots) return;
    panel_dots<R, false>(j + q * GT, m, wk.v, int(j - j0), A + j0 * lda, lda, nullptr, 0, wk.pdots + q * KP);
}

// 6: columns c > j, lane = column.  F(c, jj) finished, row j of A updated, vn1[c] downdated
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_finish_kernel(int64_t m, int64_t n, int64_t j, int64_t j0, R* A,
                                                          int64_t lda, Geqp3Work<R> wk, int nk, int ndots) {
    __shared__ R t[KP];     // V^T v
    __shared__ R Vj[KP];    // row j of V
    __shared__ R red[4][GR];
    const int jj = int(j - j0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    gather_pdots<R>(wk.pdots, ndots, KP, jj, 0, t);
    if (g == 1 && lane < jj) Vj[lane] = A[j + (j0 + lane) * lda];
    // the rows of F that belong to the columns already factored are not read again
    if (blockIdx.x == 0 && g == 2 && lane <= jj) wk.F[(j0 + lane) + int64_t(jj) * wk.ldf] = R(0);
    __syncthreads();
    const int64_t nc = n - j - 1;
    const int64_t cl = int64_t(blockIdx.x) * GR + lane, c = j + 1 + cl;
    const bool inb = c < n;
    R ys = R(0), rs = R(0);
    if (inb) {
        for (int k = g; k < nk; k += 4) ys += wk.colpart[int64_t(k) * nc + cl];
        #pragma unroll 4
        for (int k = g; k < jj; k += 4) {
            const R fk = wk.F[c + int64_t(k) * wk.ldf];
            ys -= fk * t[k];
            rs += fk * Vj[k];
        }
    }
    ys = gb_waves_sum<R>(ys, red);
    rs = gb_waves_sum<R>(rs, red);
    if (inb && g == 0) {
        const R f = wk.tau[j] * ys;
        wk.F[c + int64_t(jj) * wk.ldf] = f;
        const R a = A[j + c * lda] - rs - f;    // V(j, jj) = 1
        A[j + c * lda] = a;
        const R v1 = wk.vn1[c];
        if (v1 != R(0)) {
            R x = fabs(a) / v1;
            x = max(R(0), (R(1) + x) * (R(1) - x));
            const R q = v1 / wk.vn2[c];
            if (x * q * q <= wk.tol3z) wk.flag[c] = 1;
            else wk.vn1[c] = v1 * sqrt(x);
        }
    }
}

// 7: one workgroup per column c > j; only a flagged one works.  The updated column is stored and
// its row of F cleared, so the norm is that of the very entries the factorization goes on with:
// the trailing GEMM rounds V F^T differently, and where the column has collapsed to the size of
// that rounding a norm of other bits would misorder the pivots
template <typename R>
__global__ __launch_bounds__(GT) void geqp3_recompute_kernel(int64_t m, int64_t j, int64_t j0, R* A, int64_t lda,
                                                             Geqp3Work<R> wk) {
    __shared__ R sh[4];
    __shared__ R Fc[KP];
    const int64_t c = j + 1 + blockIdx.x;
    if (wk.flag[c] == 0) return;    // uniform over the workgroup
    const int jj = int(j - j0);
    if (int(threadIdx.x) <= jj) Fc[threadIdx.x] = wk.F[c + int64_t(threadIdx.x) * wk.ldf];
    __syncthreads();
    if (int(threadIdx.x) <= jj) wk.F[c + int64_t(threadIdx.x) * wk.ldf] = R(0);
    R s = R(0);
    for (int64_t r = j + 1 + threadIdx.x; r < m; r += GT) {
        R a = A[r + c * lda];
        for (int k = 0; k <= jj; ++k) a -= A[r + (j0 + k) * lda] * Fc[k];
        A[r + c * lda] = a;
        s += a * a;
    }
    s = gb_block_sum<R>(s, sh);
    if (threadIdx.x == 0) {
        const R nrm = sqrt(s);
        wk.vn1[c] = nrm;
        wk.vn2[c] = nrm;
        wk.recomputes[c] += 1;
        wk.flag[c] = 0;
    }
}

template <typename R>
__global__ __launch_bounds__(GT) void geqp3_scatter_rows_kernel(int64_t n, int64_t nrhs, const int64_t* jpvt,
                                                                const R* Y, int64_t ldy, R* X, int64_t ldx) {
    const int64_t i = int64_t(blockIdx.x) * GT + threadIdx.x;
    if (i >= n) return;
    const int64_t p = jpvt[i];
    if (p < 0 || p >= n) return;
    for (int64_t k = 0; k < nrhs; ++k) X[p + k * ldx] = Y[i + k * ldy];
}

}  // namespace

template <typename R>
void geqp3_norms(int64_t m, int64_t n, const R* A, int64_t lda, Geqp3Work<R> const& wk, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(geqp3_norms_kernel<R>, dim3(unsigned(n)), dim3(GT), 0, s, m, A, lda, wk);
}
template <typename R>
void geqp3_pivot(int64_t n, int64_t j, Geqp3Work<R> const& wk, hipStream_t s) {
    hipLaunchKernelGGL(geqp3_pivot_kernel<R>, dim3(1), dim3(GT), 0, s, n, j, wk);
}
template <typename R>
void geqp3_swap(int64_t m, int64_t j, int64_t j0, R* A, int64_t lda, Geqp3Work<R> const& wk, hipStream_t s) {
    hipLaunchKernelGGL(geqp3_swap_kernel<R>, dim3(gblocks_of(m)), dim3(GT), 0, s, m, j, j0, A, lda, wk);
}
template <typename R>
void geqp3_column(int64_t m, int64_t j, int64_t j0, R* A, int64_t lda, Geqp3Work<R> const& wk, hipStream_t s) {
    hipLaunchKernelGGL(geqp3_column_kernel<R>, dim3(grblocks_of(m - j)), dim3(GT), 0, s, m, j, j0, A, lda, wk);
}
template <typename R>
void geqp3_larfg(int64_t m, int64_t j, R* A, int64_t lda, Geqp3Work<R> const& wk, hipStream_t s) {
    larfg_vec<R>(m - j, A + j + j * lda, 1, wk.scal, wk.ssq, int(grblocks_of(m - j)), wk.tau + j, nullptr, wk.v + j,
                 true, s);
}
template <typename R>
void geqp3_product(int64_t m, int64_t n, int64_t j, int64_t j0, const R* A, int64_t lda, Geqp3Work<R> const& wk,
                   hipStream_t s) {
    const int64_t mr = m - j, nc = n - j - 1;
    if (mr <= 0 || nc <= 0) return;
    const int tpw = gemv_block_tpw(mr, nc);
    const int64_t nJ = (nc + TC - 1) / TC, nk = gemv_block_chunks(mr, tpw);
    const int64_t ndots = j > j0 ? gblocks_of(mr) : 0;
    hipLaunchKernelGGL(geqp3_product_kernel<R>, product_grid(nk, nJ, ndots), dim3(GT), 0, s, m, n, j, j0, A, lda, wk,
                       tpw, int(nJ), int(ndots));
}
template <typename R>
void geqp3_finish(int64_t m, int64_t n, int64_t j, int64_t j0, R* A, int64_t lda, Geqp3Work<R> const& wk,
                  hipStream_t s) {
    const int64_t mr = m - j, nc = n - j - 1;
    if (mr <= 0 || nc <= 0) return;
    const int64_t nk = gemv_block_chunks(mr, gemv_block_tpw(mr, nc));
    hipLaunchKernelGGL(geqp3_finish_kernel<R>, dim3(grblocks_of(nc)), dim3(GT), 0, s, m, n, j, j0, A, lda, wk, int(nk),
                       j > j0 ? int(gblocks_of(mr)) : 0);
}
template <typename R>
void geqp3_recompute(int64_t m, int64_t n, int64_t j, int64_t j0, R* A, int64_t lda, Geqp3Work<R> const& wk,
                     hipStream_t s) {
    const int64_t nc = n - j - 1;
    if (nc <= 0) return;
    hipLaunchKernelGGL(geqp3_recompute_kernel<R>, dim3(unsigned(nc)), dim3(GT), 0, s, m, j, j0, A, lda, wk);
}
template <typename R>
void geqp3_scatter_rows(int64_t n, int64_t nrhs, const int64_t* jpvt, const R* Y, int64_t ldy, R* X, int64_t ldx,
                        hipStream_t s) {
    if (n <= 0 || nrhs <= 0) return;
    hipLaunchKernelGGL(geqp3_scatter_rows_kernel<R>, dim3(gblocks_of(n)), dim3(GT), 0, s, n, nrhs, jpvt, Y, ldy, X,
                       ldx);
}

#define SLATE_INST_GEQP3(R)                                                                                        \
    template void geqp3_norms<R>(int64_t, int64_t, const R*, int64_t, Geqp3Work<R> const&, hipStream_t);           \
    template void geqp3_pivot<R>(int64_t, int64_t, Geqp3Work<R> const&, hipStream_t);                              \
    template void geqp3_swap<R>(int64_t, int64_t, int64_t, R*, int64_t, Geqp3Work<R> const&, hipStream_t);         \
    template void geqp3_column<R>(int64_t, int64_t, int64_t, R*, int64_t, Geqp3Work<R> const&, hipStream_t);       \
    template void geqp3_larfg<R>(int64_t, int64_t, R*, int64_t, Geqp3Work<R> const&, hipStream_t);                 \
    template void geqp3_product<R>(int64_t, int64_t, int64_t, int64_t, const R*, int64_t, Geqp3Work<R> const&,     \
                                   hipStream_t);                                                                   \
    template void geqp3_finish<R>(int64_t, int64_t, int64_t, int64_t, R*, int64_t, Geqp3Work<R> const&,            \
                                  hipStream_t);                                                                    \
    template void geqp3_recompute<R>(int64_t, int64_t, int64_t, int64_t, R*, int64_t, Geqp3Work<R> const&,         \
                                     hipStream_t);                                                                 \
    template void geqp3_scatter_rows<R>(int64_t, int64_t, const int64_t*, const R*, int64_t, R*, int64_t,          \
                                        hipStream_t);

SLATE_INST_GEQP3(float)
SLATE_INST_GEQP3(double)

}  // namespace dev
}  // namespace slate_amd
