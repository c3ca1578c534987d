// The reflector step of the one-stage reductions (hetrd.hip, gebrd.hip,
// geqp3.hip): the column kernel before it left alpha and the per-workgroup
// sums of squares of the tail; every workgroup here sums them again in the
// same order (reduce_tiles.hh), so all see the same beta, tau and scale.
#include "device_common.hh"
#include "reduce_tiles.hh"
#include "kernels.hh"

namespace slate_amd {
namespace dev {

namespace {

template <typename R>
__global__ __launch_bounds__(GT) void larfg_vec_kernel(int64_t len, R* x, int64_t incx, const R* alpha, const R* ssq,
                                                       int nssq, R* tau_out, R* beta_out, R* v, int keep_beta) {
    __shared__ R sh[4];
    const R ss = gb_partial_sum<R>(ssq, nssq, sh);
    R beta, tau, scale;
    gb_larfg<R>(alpha[0], ss, beta, tau, scale);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        tau_out[0] = tau;
        if (beta_out) beta_out[0] = beta;
    }
    const int64_t r = int64_t(blockIdx.x) * GT + threadIdx.x;
    if (r < len) {
        const R val = r == 0 ? R(1) : x[r * incx] * scale;
        x[r * incx] = r == 0 && keep_beta ? beta : val;
        v[r] = val;
    }
}

}  // namespace

template <typename R>
void larfg_vec(int64_t len, R* x, int64_t incx, const R* alpha, const R* ssq, int nssq, R* tau_out, R* beta_out, R* v,
               bool keep_beta, hipStream_t s) {
    hipLaunchKernelGGL(larfg_vec_kernel<R>, dim3(gblocks_of(len)), dim3(GT), 0, s, len, x, incx, alpha, ssq, nssq,
                       tau_out, beta_out, v, keep_beta ? 1 : 0);
}

template void larfg_vec<float>(int64_t, float*, int64_t, const float*, const float*, int, float*, float*, float*, bool,
                               hipStream_t);
template void larfg_vec<double>(int64_t, double*, int64_t, const double*, const double*, int, double*, double*,
                                double*, bool, hipStream_t);

}  // namespace dev
}  // namespace slate_amd
