// Placement of the factors of the bidiagonal divide and conquer (src/bdsdc.cc;
// its merge kernels are kernels/dc_merge.hip):
//   * bdsdc_place: real factor -> (block-cyclic local part of) a matrix of
//     the caller's type, optionally transposed and with a row phase.
#include "device_common.hh"
#include "kernels.hh"

namespace slate_amd {
namespace dev {

namespace {

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
