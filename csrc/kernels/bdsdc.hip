// Device side of the bidiagonal divide and conquer (src/bdsdc.cc; the
// Gu-Eisenstat merge that LAPACK's lasd4 / lasd8 / lasd3 implement, written
// from the math).
//
// One merge, after sorting and deflation on the host, is the SVD of
//   M = [ z^T ; 0 diag(d_2 .. d_k) ],  0 = d_1 < d_2 < ... < d_k,
// whose singular values are the roots of
//   f(sigma) = 1 + sum_i z_i^2 / ((d_i - sigma)(d_i + sigma)).
//   * bdsdc_secular_roots: one WAVE per root.  The equation is solved in
//     sigma^2 by the rational iteration of slate_amd/secular.hh (root_core)
//     with poles d_i^2 that exist only as differences
//     (d_i - d_o)(d_i + d_o); the O(k) sums of an iteration are split over
//     the lanes and reduced by an xor butterfly.  The converged shift
//     t = sigma^2 - d_o^2 becomes tau = sigma - d_o = t / (sigma + d_o), so
//     d_i - sigma_j = (d_i - d_o) - tau_j keeps full relative precision.
//   * bdsdc_zhat: z recomputed from the roots (Loewner), one thread per i.
//   * bdsdc_merge_matrices: one workgroup per output column of MU (left,
//     N x N) or MV (right, (N + sqre) x (N + sqre)): the normalised secular
//     vector or a deflated unit vector in the sorted basis, the recorded
//     deflation rotations in reverse, the (q1, q2) rotation on the right
//     side, scattered through the sort permutation into column-major M.
//   * bdsdc_place: real factor -> (block-cyclic local part of) a matrix of
//     the caller's type, optionally transposed and with a row phase.
#include "device_common.hh"
#include "kernels.hh"
#include "slate_amd/secular.hh"

namespace slate_amd {
namespace dev {

namespace {

__global__ __launch_bounds__(256) void bdsdc_secular_roots_kernel(int64_t k, const double* dd, const double* zz,
                                                                 double znorm2, int64_t* org, double* tau) {
    const int lane = threadIdx.x & 63;
    const int64_t j = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (j >= k) return;   // wave-uniform
    auto wsum = [&](int64_t o, double t) {
        slate::secular::Sums<double> s;
        const double d0 = dd[o];
        for (int64_t i = lane; i < k; i += 64) {
            const double r = zz[i] / ((dd[i] - d0) * (dd[i] + d0) - t);
            if (i <= j) { s.psi += zz[i] * r; s.dpsi += r * r; }
            else { s.phi += zz[i] * r; s.dphi += r * r; }
        }
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
    auto diff = [dd](int64_t i, int64_t o) { return (dd[i] - dd[o]) * (dd[i] + dd[o]); };
    int64_t o2 = j;
    const double t = slate::secular::root_core<double>(k, j, 1.0, znorm2, &o2, diff, wsum);
    if (lane == 0) {
        org[j] = o2;
        tau[j] = slate::secular::sqrt_shift(dd[o2], t);
    }
}

__global__ __launch_bounds__(64) void bdsdc_zhat_kernel(int64_t k, const double* dd, const double* zz,
                                                        const int64_t* org, const double* tau, double* zh) {
    const int64_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= k) return;
    const double di = dd[i];
    // (sigma_j - d_i)(sigma_j + d_i)
    auto lmd = [&](int64_t j) {
        const double dorg = dd[org[j]];
        return ((dorg - di) + tau[j]) * ((dorg + di) + tau[j]);
    };
    double pr = lmd(k - 1);
    for (int64_t j = 0; j < k - 1; ++j) {
        const double dj = (j < i) ? dd[j] : dd[j + 1];
        pr *= lmd(j) / ((dj - di) * (dj + di));
    }
    zh[i] = copysign(sqrt(fabs(pr)), zz[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void bdsdc_merge_matrices_kernel(BdsdcMerge a, int vside, int64_t c_first, T* M,
                                                                   int64_t ldm, double* scratch) {
    const int64_t jo = c_first + blockIdx.x;                  // output column
    const int64_t rows = a.n + (vside ? a.sqre : 0);
    double* vec = scratch + blockIdx.x * a.n;                 // sorted basis, a.n entries
    __shared__ double red[256];
    if (jo >= a.n) {
        // right side, sqre = 1: the surviving null vector -qs q1 + qc q2
        for (int64_t r = threadIdx.x; r < rows; r += 256)
            M[r + jo * ldm] = T(r == a.nl ? -a.qs : (r == a.n ? a.qc : 0.0));
        return;
    }
    for (int64_t s = threadIdx.x; s < a.n; s += 256) vec[s] = 0.0;
    __syncthreads();
    const int64_t r = a.ord[jo];
    if (r < a.k) {
        const double dr = a.dd[a.org[r]], tr = a.tau[r];
        double part = 0;
        for (int64_t i = threadIdx.x; i < a.k; i += 256) {
            const double di = a.dd[i];
            double u = a.zh[i] / (((di - dr) - tr) * ((di + dr) + tr));
            if (!vside) u = (i == 0) ? -1.0 : di * u;
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
        const int64_t nrot = vside ? a.nrot_v : a.nrot_u;
        const int64_t* rab = vside ? a.rot_ab_v : a.rot_ab_u;
        const double* rcs = vside ? a.rot_cs_v : a.rot_cs_u;
        for (int64_t t = nrot - 1; t >= 0; --t) {
            const int64_t x = rab[2 * t], y = rab[2 * t + 1];
            const double c = rcs[2 * t], sn = rcs[2 * t + 1];
            const double vx = vec[x], vy = vec[y];
            vec[x] = c * vx - sn * vy;
            vec[y] = sn * vx + c * vy;
        }
    }
    __syncthreads();
    // row r of the block takes sorted entry inv_perm[r]; on the right side the
    // special entry (sorted index 0, row nl) is the coefficient of
    // qc q1 + qs q2, and q2 is row n
    for (int64_t row = threadIdx.x; row < rows; row += 256) {
        double v;
        if (row == a.n) v = a.qs * vec[0];
        else {
            v = vec[a.inv_perm[row]];
            if (vside && row == a.nl) v *= a.qc;
        }
        M[row + jo * ldm] = T(v);
    }
}

template <typename T, typename R>
__global__ __launch_bounds__(256) void bdsdc_place_kernel(BdsdcPlace p, const R* src, int64_t lds, const T* phase, T* dst,
                                                          int64_t ldd) {
    const int64_t lr = int64_t(blockIdx.y) * 256 + threadIdx.x, lc = blockIdx.x;
    if (lr >= p.lrows) return;
    const int64_t gi = ((lr / p.mb) * p.p + p.rrel) * p.mb + lr % p.mb;
    const int64_t gj = ((lc / p.nb) * p.q + p.crel) * p.nb + lc % p.nb;
    if (gi >= p.m || gj >= p.n) return;
    const R v = p.trans ? src[gj + gi * lds] : src[gi + gj * lds];
    if constexpr (is_cplx<T>::value) {
        T out = T(v, R(0));
        if (phase) out = phase[gi] * v;
        dst[lr + lc * ldd] = out;
    } else {
        dst[lr + lc * ldd] = phase ? phase[gi] * v : v;
    }
}

}  // namespace

void bdsdc_secular_roots(int64_t k, const double* dd, const double* zz, double znorm2, int64_t* org, double* tau,
                         hipStream_t s) {
    if (k <= 0) return;
    hipLaunchKernelGGL(bdsdc_secular_roots_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, s, k, dd, zz, znorm2,
                       org, tau);
}

void bdsdc_zhat(int64_t k, const double* dd, const double* zz, const int64_t* org, const double* tau, double* zh,
                hipStream_t s) {
    if (k <= 0) return;
    hipLaunchKernelGGL(bdsdc_zhat_kernel, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, k, dd, zz, org, tau, zh);
}

template <typename T>
void bdsdc_merge_matrices(BdsdcMerge const& m, bool vside, int64_t c_first, int64_t ncols, T* M, int64_t ldm,
                          double* scratch, hipStream_t s) {
    if (ncols <= 0) return;
    hipLaunchKernelGGL(bdsdc_merge_matrices_kernel<T>, dim3((unsigned)ncols), dim3(256), 0, s, m, vside ? 1 : 0,
                       c_first, M, ldm, scratch);
}
template void bdsdc_merge_matrices<double>(BdsdcMerge const&, bool, int64_t, int64_t, double*, int64_t, double*,
                                           hipStream_t);
template void bdsdc_merge_matrices<float>(BdsdcMerge const&, bool, int64_t, int64_t, float*, int64_t, double*,
                                          hipStream_t);

template <typename T>
void bdsdc_place(BdsdcPlace const& p, const rt<T>* src, int64_t lds, const T* phase, T* dst, int64_t ldd,
                 hipStream_t s) {
    if (p.lrows <= 0 || p.lcols <= 0) return;
    hipLaunchKernelGGL((bdsdc_place_kernel<T, rt<T>>), dim3((unsigned)p.lcols, (unsigned)((p.lrows + 255) / 256)),
                       dim3(256), 0, s, p, src, lds, phase, dst, ldd);
}
template void bdsdc_place<float>(BdsdcPlace const&, const float*, int64_t, const float*, float*, int64_t, hipStream_t);
template void bdsdc_place<double>(BdsdcPlace const&, const double*, int64_t, const double*, double*, int64_t,
                                  hipStream_t);
template void bdsdc_place<cplx<float>>(BdsdcPlace const&, const float*, int64_t, const cplx<float>*, cplx<float>*,
                                       int64_t, hipStream_t);
template void bdsdc_place<cplx<double>>(BdsdcPlace const&, const double*, int64_t, const cplx<double>*, cplx<double>*,
                                        int64_t, hipStream_t);

}  // namespace dev
}  // namespace slate_amd
