// Device side of one merge of the divide and conquer, tridiagonal (stedc_dist,
// eig_dist.cc; reference src/stedc_secular.cc, stedc_merge.cc, LAPACK laed3 /
// laed4 semantics) and bidiagonal (bdsdc.cc; what LAPACK's lasd4 / lasd8 /
// lasd3 implement, written from the math).  Host side and host twins:
// src/dc_merge.cc.
//
// After sorting and deflation on the host (O(n)) a merge is a rank-one
// modified diagonal with k active poles.  The two problems differ in the pole
// family (slate_amd/secular.hh) and in where a column of the merge matrix
// lands (the side policies of kernels.hh):
//   * stedc, LinearPoles: D + rho z z^T, root lambda_j = dd[org_j] + tau_j;
//     every rank builds ONLY its block-cyclic local entries of the n x n
//     merge matrix M (Q_new = Q_old M);
//   * bdsdc, SquaredPoles: M = [ z^T ; 0 diag(d_2 .. d_k) ], 0 = d_1 < d_2 <
//     ..., singular values the roots of
//     f(sigma) = 1 + sum_i z_i^2 / ((d_i - sigma)(d_i + sigma)), solved in
//     sigma^2 with poles d_i^2 that exist only as differences
//     (d_i - d_o)(d_i + d_o); the converged shift becomes
//     tau = sigma - d_o, so d_i - sigma_j = (d_i - d_o) - tau_j keeps full
//     relative precision; dense MU (N x N) and MV ((N + sqre) square).
// Kernels:
//   * secular_roots: one WAVE per root, the rational iteration of secular.hh
//     to full relative precision of tau_j (distance to the nearest pole),
//     which the Gu-Eisenstat vectors need;
//   * zhat: z recomputed from the computed roots (Loewner), one thread per i;
//   * merge_column: one workgroup per output column forms the column in the
//     sorted basis (normalised secular vector, or a unit vector for a
//     deflated column), applies the recorded deflation rotations in reverse
//     order and scatters it through the sort permutation.  The product with
//     the old vectors is the MFMA GEMM.
#include "device_common.hh"
#include "kernels.hh"

namespace slate_amd {
namespace dev {

namespace {

// One WAVE per root: the O(k) sums of every iteration are split over the
// 64 lanes and reduced by an xor butterfly, then lane 0's totals are
// broadcast so every lane runs the identical (uniform) iteration.  A thread
// per root left k / 64 waves for the whole chip with each lane walking all k
// poles per iteration (7x slower, profiles/r4_secular_wave_ab.txt).
template <typename Poles>
__global__ __launch_bounds__(256) void secular_roots_kernel(Poles poles, int64_t k, double rho, const double* zz,
                                                           double znorm2, int64_t* org, double* tau) {
    const int lane = threadIdx.x & 63;
    const int64_t j = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (j >= k) return;   // wave-uniform
    auto wsum = [&](int64_t o, double t) {
        slate::secular::Sums<double> s = slate::secular::partial_sums<double>(poles, k, j, zz, o, t, lane, 64);
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s.psi += __shfl_xor(s.psi, off);
            s.phi += __shfl_xor(s.phi, off);
            s.dpsi += __shfl_xor(s.dpsi, off);
            s.dphi += __shfl_xor(s.dphi, off);
        }
        s.psi = __shfl(s.psi, 0);
        s.phi = __shfl(s.phi, 0);
        s.dpsi = __shfl(s.dpsi, 0);
        s.dphi = __shfl(s.dphi, 0);
        return s;
    };
    int64_t o2 = j;
    const double t = slate::secular::root_of<double>(poles, k, j, rho, znorm2, &o2, wsum);
    if (lane == 0) {
        org[j] = o2;
        tau[j] = t;
    }
}

template <typename Poles>
__global__ __launch_bounds__(64) void zhat_kernel(Poles poles, int64_t k, double rho, const double* zz,
                                                  const int64_t* org, const double* tau, double* zh) {
    const int64_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= k) return;
    zh[i] = slate::secular::zhat_entry<double>(poles, k, i, rho, zz, org, tau);
}

// vec is per-workgroup global scratch (a.n doubles): the column in the sorted basis
template <typename T, typename Side>
__global__ __launch_bounds__(256) void merge_column_kernel(DcMerge a, DcRotations rot, Side side, int64_t c_first, T* M,
                                                           int64_t ldm, double* scratch) {
    const int64_t col = c_first + blockIdx.x;                 // output column
    const int64_t jo = side.result(col), rows = side.rows(a.n);
    T* out = M + col * ldm;
    double* vec = scratch + blockIdx.x * a.n;
    __shared__ double red[256];
    if (jo >= a.n) {
        for (int64_t r = threadIdx.x; r < rows; r += 256) out[r] = T(side.null_entry(r, a.n));
        return;
    }
    for (int64_t s = threadIdx.x; s < a.n; s += 256) vec[s] = 0.0;
    __syncthreads();
    const int64_t r = a.ord[jo];
    if (r < a.k) {
        const typename Side::Poles poles{a.dd};
        const double dr = a.dd[a.org[r]], tr = a.tau[r];
        double part = 0;
        for (int64_t i = threadIdx.x; i < a.k; i += 256) {
            const double u = side.entry(i, a.dd[i], a.zh[i] / poles.pole_minus_root(i, dr, tr));
            vec[a.act[i]] = u;
            part += u * u;
        }
        red[threadIdx.x] = part;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        const double inv = 1.0 / sqrt(red[0]);
        for (int64_t i = threadIdx.x; i < a.k; i += 256) vec[a.act[i]] *= inv;
    } else if (threadIdx.x == 0) {
        vec[a.defl[r - a.k]] = 1.0;
    }
    __syncthreads();
    // G w with G = G_1 ... G_t: the last rotation acts first
    if (threadIdx.x == 0) {
        for (int64_t t = rot.nrot - 1; t >= 0; --t) {
            const int64_t x = rot.ab[2 * t], y = rot.ab[2 * t + 1];
            const double c = rot.cs[2 * t], sn = rot.cs[2 * t + 1];
            const double vx = vec[x], vy = vec[y];
            vec[x] = c * vx - sn * vy;
            vec[y] = sn * vx + c * vy;
        }
    }
    __syncthreads();
    for (int64_t row = threadIdx.x; row < rows; row += 256) out[row] = T(side.row_entry(row, a.n, vec, a.inv_perm));
}

}  // namespace

template <typename Poles>
void secular_roots(Poles poles, int64_t k, double rho, const double* zz, double znorm2, int64_t* org, double* tau,
                   hipStream_t s) {
    if (k <= 0) return;
    hipLaunchKernelGGL(secular_roots_kernel<Poles>, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, s, poles, k, rho, zz,
                       znorm2, org, tau);
}

template <typename Poles>
void zhat(Poles poles, int64_t k, double rho, const double* zz, const int64_t* org, const double* tau, double* zh,
          hipStream_t s) {
    if (k <= 0) return;
    hipLaunchKernelGGL(zhat_kernel<Poles>, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, poles, k, rho, zz, org, tau,
                       zh);
}

template <typename T, typename Side>
void merge_columns(DcMerge const& m, DcRotations const& rot, Side const& side, int64_t c_first, int64_t ncols, T* M,
                   int64_t ldm, double* scratch, hipStream_t s) {
    if (ncols <= 0) return;
    hipLaunchKernelGGL((merge_column_kernel<T, Side>), dim3((unsigned)ncols), dim3(256), 0, s, m, rot, side, c_first, M,
                       ldm, scratch);
}

#define SLATE_DC_POLES_INST(P)                                                                               \
    template void secular_roots<P>(P, int64_t, double, const double*, double, int64_t*, double*, hipStream_t); \
    template void zhat<P>(P, int64_t, double, const double*, const int64_t*, const double*, double*, hipStream_t);
SLATE_DC_POLES_INST(slate::secular::LinearPoles<double>)
SLATE_DC_POLES_INST(slate::secular::SquaredPoles<double>)
#define SLATE_DC_COLUMNS_INST(T, S)                                                                         \
    template void merge_columns<T, S>(DcMerge const&, DcRotations const&, S const&, int64_t, int64_t, T*, int64_t, \
                                      double*, hipStream_t);
SLATE_DC_COLUMNS_INST(double, StedcSide)
SLATE_DC_COLUMNS_INST(float, StedcSide)
SLATE_DC_COLUMNS_INST(double, BdsdcSide)
SLATE_DC_COLUMNS_INST(float, BdsdcSide)

}  // namespace dev
}  // namespace slate_amd
