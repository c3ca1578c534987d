// Split-operand bf16 MFMA GEMM for gfx950:
//   C = alpha * op(A) * op(B) + beta * C,  fp32 in memory, column-major.
//
// gfx950 has no xf32 path and v_mfma_f32_16x16x4_f32 runs at 1/16 of the bf16
// MFMA rate, so an fp32 product is formed here from bf16 MFMAs with fp32
// accumulation.  Each operand element x is split ONCE, while its tile is
// staged, into NS bf16 planes
//     x0 = bf16_rne(x),  x1 = bf16_rne(x - x0),  x2 = bf16_rne(x - x0 - x1)
// (the subtractions are exact in fp32), and the kernel issues the plane
// products (i, j) with i + j < NS: 1 (bf16), 3 (bf16x3) or 6 (bf16x6) MFMAs per
// K-step, smallest terms first.
//
//  * 128 x 128 C tile per 256-thread workgroup (4 waves, 2 x 2), 64 x 64 per
//    wave = 2 x 2 tiles of v_mfma_f32_32x32x16_bf16, BK = 32.
//  * global fp32 (16-B loads along the contiguous dimension) -> registers ->
//    convert + split -> LDS as bf16 planes.  An M- / N-contiguous operand is
//    transposed in registers (a 4 x 4 block per thread) on its way in, so every
//    LDS image is [row][k] with K contiguous and a lane's 8-element MFMA
//    fragment is one 16-B LDS read.
//  * LDS rows are 32 bf16 + 8 pad = 80 B: the 16-B slot of row r is 5r mod 16,
//    distinct over 16 consecutive rows, and the 8-B staging writes of a wave
//    spread evenly over the 32 write banks.
//  * LDS double buffer, one barrier per K-tile, and a register prefetch two
//    K-tiles deep (two register sets): with one or two workgroups per CU the
//    load latency does not hide behind a single tile's MFMAs (measured on
//    32768^2 x 1024: bf16 8.8 -> 7.3 ms).  The split's VALU work interleaves
//    with the second k-step's MFMAs.  NS = 3 uses 120 KB of LDS (one
//    workgroup per CU), NS = 1 / 2 use 40 / 80 KB.
//  * Operands are swapped in the MFMA (D = op(B)^T op(A)^T) so the
//    accumulator's lane index runs along M: 32 lanes store 128 contiguous bytes
//    of a column of C.
//  * XCD-aware grouped tile order as in gemm_mfma.hip.
//
// Inf / NaN inputs come out as NaN (inf - bf16(inf) is NaN in the lower planes).
#include "device_common.hh"
#include "kernels.hh"

#include <type_traits>

namespace slate_amd {
namespace dev {

namespace {

using bf16x4_t = __bf16 __attribute__((ext_vector_type(4)));
using bf16x8_t = __bf16 __attribute__((ext_vector_type(8)));
using f32x4_t  = float __attribute__((ext_vector_type(4)));
using f32x16_t = float __attribute__((ext_vector_type(16)));

constexpr int kBT   = 128;            // C tile edge (BM == BN)
constexpr int kBK   = 32;             // K-tile
constexpr int kNT   = 256;            // threads per workgroup
constexpr int kRow  = kBK + 8;        // LDS row stride in bf16 elements (80 B)
constexpr int kPlane = kBT * kRow;    // one plane of one operand, bf16 elements

// Split four fp32 values into NS bf16 planes.
template <int NS>
__device__ __forceinline__ void split4(const float (&v)[4], bf16x4_t (&out)[NS]) {
    #pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = v[e];
        #pragma unroll
        for (int p = 0; p < NS; ++p) {
            const __bf16 b = (__bf16)x;
            out[p][e] = b;
            if (p + 1 < NS) x -= (float)b;
        }
    }
}

// One 128 x 32 operand tile: registers <- global, LDS planes <- registers.
// Element (x, kk) of the operand is X[kk + x*ld] (KCONTIG) or X[x + kk*ld].
template <int NS, bool KCONTIG>
struct Stager {
    float r[4][4];
    int x_, k_;    // KCONTIG: row x_ + 32 i, k = k_ .. k_+3;  else rows x_ .. x_+3, k = k_ + i

    __device__ __forceinline__ void init() {
        const int tid = threadIdx.x;
        if constexpr (KCONTIG) {
            k_ = 4 * (tid & 7);
            x_ = tid >> 3;
        } else {
            // 8 row-quads x 8 k-quads per wave: 128-B global segments per k, and
            // LDS writes that cover every bank
            x_ = 4 * ((tid & 7) + 8 * (tid >> 6));
            k_ = 4 * ((tid >> 3) & 7);
        }
    }

    /// Vector loads only (tile fully inside the operand, 16-B aligned).
    __device__ __forceinline__ void load_fast(const float* __restrict__ X, int64_t ld, int64_t x0, int64_t k0) {
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* p = KCONTIG ? X + (k0 + k_) + (x0 + x_ + 32 * i) * ld
                                     : X + (x0 + x_) + (k0 + k_ + i) * ld;
            const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p);
            r[i][0] = t[0]; r[i][1] = t[1]; r[i][2] = t[2]; r[i][3] = t[3];
        }
    }

    /// Edge tiles: every element loaded from an index clamped into the operand
    /// (xdim, kdim >= 1) and zeroed outside it, so no load sits behind a branch.
    __device__ __forceinline__ void load_checked(const float* __restrict__ X, int64_t ld, int64_t x0, int64_t k0,
                                                 int64_t xdim, int64_t kdim) {
        #pragma unroll
        for (int i = 0; i < 4; ++i)
            #pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t gx = x0 + x_ + (KCONTIG ? 32 * i : e);
                const int64_t gk = k0 + k_ + (KCONTIG ? e : i);
                const int64_t cx = min(gx, xdim - 1), ck = min(gk, kdim - 1);
                const float v = KCONTIG ? X[ck + cx * ld] : X[cx + ck * ld];
                r[i][e] = (gx < xdim && gk < kdim) ? v : 0.f;
            }
    }

    // L: this operand's NS planes in one LDS buffer
    __device__ __forceinline__ void store(__bf16* L) const {
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[4];
            int row;
            if constexpr (KCONTIG) {
                #pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = r[i][e];
                row = x_ + 32 * i;
            } else {
                #pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = r[e][i];
                row = x_ + i;
            }
            bf16x4_t pl[NS];
            split4<NS>(v, pl);
            #pragma unroll
            for (int p = 0; p < NS; ++p)
                *reinterpret_cast<bf16x4_t*>(L + p * kPlane + row * kRow + k_) = pl[p];
        }
    }
};

// Tile order: XCD-aware bijective remap, then GROUP tile-rows at a time.
__device__ __forceinline__ void tile_coords(int mt, int nt, int& tm, int& tn) {
    const int nblk = mt * nt;
    const int bid = xcd_remap(blockIdx.x, nblk);
    constexpr int GROUP = 8;
    const int group = bid / (GROUP * nt);
    const int first_m = group * GROUP;
    const int gsize = min(mt - first_m, GROUP);
    const int within = bid % (GROUP * nt);
    tm = first_m + within % gsize;
    tn = within / gsize;
}

// uplo: 'G' full C; 'L' / 'U' only that triangle of a square C.
template <int NS, bool A_KC, bool B_KC>
__global__ __launch_bounds__(kNT)
void gemm_bf16s_kernel(char uplo, int64_t m, int64_t n, int64_t k, float alpha,
                       const float* __restrict__ A, int64_t lda,
                       const float* __restrict__ B, int64_t ldb,
                       float beta, float* __restrict__ C, int64_t ldc, bool aligned)
{
    constexpr int OPER = NS * kPlane;          // one operand's planes
    constexpr int BUF  = 2 * OPER;             // A planes, then B planes
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * BUF];

    const int mt = (int)((m + kBT - 1) / kBT), nt = (int)((n + kBT - 1) / kBT);
    int tm, tn;
    tile_coords(mt, nt, tm, tn);
    // tiles wholly outside the triangle do nothing
    if (uplo == 'L' && tm < tn) return;
    if (uplo == 'U' && tm > tn) return;
    const int64_t m0 = (int64_t)tm * kBT, n0 = (int64_t)tn * kBT;

    const int lane = threadIdx.x & 63;
    const int wid  = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;

    f32x16_t acc[2][2];
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < 2; ++j)
            #pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // two register sets: tile kt + 2 is loaded while tile kt is multiplied and
    // tile kt + 1 (loaded one iteration earlier) is split into LDS
    Stager<NS, A_KC> sa0, sa1;
    Stager<NS, B_KC> sb0, sb1;
    sa0.init(); sa1.init();
    sb0.init(); sb1.init();
    const int KT = (int)((k + kBK - 1) / kBK);
    // Interior tiles (the common case) run a K loop with vector loads only;
    // edge tiles, a K remainder and unaligned operands take the checked loop.
    // Two loops, not a branch per load: a load behind a branch is waited for
    // at the branch's end, which would expose the whole load latency.
    auto kloop = [&](auto interior_tag) {
    constexpr bool INTERIOR = decltype(interior_tag)::value;
    // Prefetches are unconditional: a tile index past the end is clamped to
    // the last tile (interior) or reads as zeros (checked); it is never stored.
    auto load_tiles = [&](Stager<NS, A_KC>& sa, Stager<NS, B_KC>& sb, int t) {
        if constexpr (INTERIOR) {
            const int64_t k0 = (int64_t)min(t, KT - 1) * kBK;
            sa.load_fast(A, lda, m0, k0);
            sb.load_fast(B, ldb, n0, k0);
        } else {
            const int64_t k0 = (int64_t)t * kBK;
            sa.load_checked(A, lda, m0, k0, m, k);
            sb.load_checked(B, ldb, n0, k0, n, k);
        }
    };
    if (KT > 0) {
        load_tiles(sa0, sb0, 0);
        load_tiles(sa1, sb1, 1);
        sa0.store(smem);
        sb0.store(smem + OPER);
        __syncthreads();
    }

    // lane (r = lane & 31, h = lane >> 5) holds k = 8h .. 8h+7 of row r of a
    // 32-row operand block, for the A and the B operand of the MFMA alike
    const int frag_off = (lane & 31) * kRow + 8 * (lane >> 5);

    // k-steps [s0, s1) of 16 of the tile in buffer cur
    auto compute = [&](int cur, int s0, int s1) {
        const __bf16* As = smem + cur * BUF + (wm * 64) * kRow + frag_off;
        const __bf16* Bs = smem + cur * BUF + OPER + (wn * 64) * kRow + frag_off;
        #pragma unroll
        for (int s = s0; s < s1; ++s) {
            bf16x8_t fa[NS][2], fb[NS][2];
            #pragma unroll
            for (int p = 0; p < NS; ++p)
                #pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[p][i] = *reinterpret_cast<const bf16x8_t*>(As + p * kPlane + i * 32 * kRow + s * 16);
                    fb[p][i] = *reinterpret_cast<const bf16x8_t*>(Bs + p * kPlane + i * 32 * kRow + s * 16);
                }
            // plane products with pa + pb == t, smallest terms first
            #pragma unroll
            for (int t = NS - 1; t >= 0; --t)
                #pragma unroll
                for (int pa = 0; pa <= t; ++pa)
                    #pragma unroll
                    for (int i = 0; i < 2; ++i)
                        #pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[t - pa][j], fa[pa][i], acc[i][j],
                                                                                0, 0, 0);
        }
    };
    // One K-tile: prefetch tile kt + 2 into (la, lb), multiply tile kt, split
    // tile kt + 1 from (ta, tb) into the other LDS buffer.  The last K-tile is
    // peeled off, so nothing here sits under a branch (a load under a branch is
    // waited for where the branch ends, before the MFMAs it should hide behind).
    auto step = [&](Stager<NS, A_KC>& la, Stager<NS, B_KC>& lb, Stager<NS, A_KC> const& ta,
                    Stager<NS, B_KC> const& tb, int kt) {
        const int cur = kt & 1;
        load_tiles(la, lb, kt + 2);
        // Keep the prefetch issued ahead of this tile's MFMAs, and the split +
        // LDS stores behind the first k-step's: the scheduler otherwise sinks
        // loads to where they are consumed and waits for them at once.  The
        // split's VALU work is left free to interleave with the second
        // k-step's MFMAs.
        __builtin_amdgcn_sched_barrier(0);
        compute(cur, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        compute(cur, 1, kBK / 16);
        __bf16* nxt = smem + (cur ^ 1) * BUF;
        ta.store(nxt);
        tb.store(nxt + OPER);
        __syncthreads();
    };
    int kt = 0;
    for (; kt + 2 < KT; kt += 2) {
        step(sa0, sb0, sa1, sb1, kt);
        step(sa1, sb1, sa0, sb0, kt + 1);
    }
    if (kt + 1 < KT) step(sa0, sb0, sa1, sb1, kt);
    if (KT > 0) compute((KT - 1) & 1, 0, kBK / 16);
    };
    if (aligned && m0 + kBT <= m && n0 + kBT <= n && k % kBK == 0) kloop(std::true_type{});
    else kloop(std::false_type{});

    // epilogue: acc[i][j] is D[n][m] of v_mfma_f32_32x32x16: column (lane & 31)
    // runs along M, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) along N
    const bool beta_zero = (beta == 0.f);
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t gm = m0 + wm * 64 + i * 32 + (lane & 31);
        #pragma unroll
        for (int j = 0; j < 2; ++j) {
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gn = n0 + wn * 64 + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                bool in = gm < m && gn < n;
                if (uplo == 'L') in = in && gm >= gn;
                if (uplo == 'U') in = in && gm <= gn;
                if (in) {
                    float v = alpha * acc[i][j][r];
                    if (!beta_zero) v += beta * C[gm + gn * ldc];
                    C[gm + gn * ldc] = v;
                }
            }
        }
    }
}

template <int NS, bool A_KC, bool B_KC>
void launch_bf16s(char uplo, int64_t m, int64_t n, int64_t k, float alpha, const float* A, int64_t lda,
                  const float* B, int64_t ldb, float beta, float* C, int64_t ldc, hipStream_t stream) {
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; };
    const bool aligned = al(A) && al(B) && lda % 4 == 0 && ldb % 4 == 0;
    const int64_t mt = (m + kBT - 1) / kBT, nt = (n + kBT - 1) / kBT;
    hipLaunchKernelGGL((gemm_bf16s_kernel<NS, A_KC, B_KC>), dim3((unsigned)(mt * nt)), dim3(kNT), 0, stream,
                       uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, aligned);
}

template <int NS>
void dispatch_bf16s(char uplo, bool a_kc, bool b_kc, int64_t m, int64_t n, int64_t k, float alpha, const float* A,
                    int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc, hipStream_t s) {
    if (a_kc && b_kc) launch_bf16s<NS, true, true>(uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
    else if (a_kc)    launch_bf16s<NS, true, false>(uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
    else if (b_kc)    launch_bf16s<NS, false, true>(uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
    else              launch_bf16s<NS, false, false>(uplo, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, s);
}

}  // namespace

void gemm_bf16s(int nsplit, char uplo, char transA, char transB, int64_t m, int64_t n, int64_t k,
                float alpha, const float* A, int64_t lda, const float* B, int64_t ldb,
                float beta, float* C, int64_t ldc, hipStream_t stream)
{
    if (m <= 0 || n <= 0) return;
    if (k < 0) k = 0;
    if (uplo != 'L' && uplo != 'U') uplo = 'G';
    // op(A) = A: contiguous along M; op(A) = A^T: contiguous along K.
    // op(B) = B: contiguous along K; op(B) = B^T: contiguous along N.
    const bool a_kc = (transA != 'N'), b_kc = (transB == 'N');
    switch (nsplit) {
        case 1:  dispatch_bf16s<1>(uplo, a_kc, b_kc, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, stream); break;
        case 2:  dispatch_bf16s<2>(uplo, a_kc, b_kc, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, stream); break;
        default: dispatch_bf16s<3>(uplo, a_kc, b_kc, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, stream); break;
    }
}

}  // namespace dev
}  // namespace slate_amd
