// The split-fp16 layer GEMM of the texture network and its packed weight image: what the tile skeleton (texture_tile.h) and
// the pack kernels of texture.hip and texgrad.hip (the reverse sweep runs the same GEMM on transposed images) share.
#pragma once
#include "idr_common.h"
#include "mfma_split.h"
#include "texture_common.h"

static_assert(kAP == 2, "the texture kernels are written for the two-part fp16 layout");

namespace {

constexpr int kTexAD = 2;            // weight fragments requested two K-steps ahead (idr_x16.hip)
constexpr int kTexHdr = 64;          // header floats: [0..7] 2^s_l | [16..23] rowsum_l | [32..39] max|b_l|

// packed (floats): header kTexHdr | bias_k n_layers*H (K-order) | head 3*H (K-order rows) | head bias 4 |
//   FW16_0 K0*H | per l = 1..n_layers-1: FW16_l H*H
// FW16: uint4 index ((s*NTO + To)*2 + part)*64 + lane as in siren_common.h.
__host__ __device__ inline int64_t texp_bias(const TexShape& s, int l) { return kTexHdr + (int64_t)l * s.H; }
__host__ __device__ inline int64_t texp_head(const TexShape& s) { return texp_bias(s, s.n_layers); }
__host__ __device__ inline int64_t texp_hbias(const TexShape& s) { return texp_head(s) + 3 * (int64_t)s.H; }
__host__ __device__ inline int64_t texp_fw0(const TexShape& s) { return texp_hbias(s) + 4; }
__host__ __device__ inline int64_t texp_fw(const TexShape& s, int l) {     // l >= 1
  return texp_fw0(s) + (int64_t)s.K0 * s.H + (int64_t)(l - 1) * s.H * s.H;
}
__host__ __device__ inline int64_t texp_end(const TexShape& s) { return texp_fw(s, s.n_layers); }

__host__ __device__ inline int tex_feat_of_ko(int64_t ko) { return x3_feat((int)(ko >> 4), 8 * (int)((ko >> 3) & 1) + (int)(ko & 7)); }

// one 32-bit word of a split-fp16 image: two neighbouring values (already under the layer's scale) as two halves, part 0
// their fp16 roundings, part 1 what the roundings left
__device__ __forceinline__ unsigned tex_f16_word(f32x2 v, int part) {
  const f16x2 h = __builtin_convertvector(v, f16x2);
  const f16x2 lo = __builtin_convertvector(v - __builtin_convertvector(h, f32x2), f16x2);
  return part == 0 ? __builtin_bit_cast(unsigned, h) : __builtin_bit_cast(unsigned, lo);
}

// The layer GEMM in THREE passes over K, one partial product each, smallest first: W_l x_h, W_h x_l (each 2^-11 of the
// result), then W_h x_h.  With all three in one pass (gemm_x3) every 16-term MFMA rounds the accumulator at the magnitude
// of the result, three times per K-step; here the small products are rounded at the bias's magnitude or their own and the
// result's magnitude sees ONE rounding per K-step.  Measured against float64 that accumulation was the larger part of the
// kernel's error (profiles/texture_float64_margin.txt).  The price: three operand parts are read per K-step
// where gemm_x3 reads two (a pass requests only the one part of each operand it multiplies, which also keeps a fragment
// set at a quarter of gemm_x3's registers).
// Fragment pipeline as gemm_x3's: sets of A requested KAD K-steps ahead, A[0..KAD-1] hold the first fragments on entry and
// those of the next stage (next_imgw, next_s, part next_a_part) on exit; activations one K-step ahead.
// a_part / b_part: the part (0 high, 1 low) of the weight image / of the activations this pass multiplies.
constexpr int kTexQA[3] = {1, 0, 0};
constexpr int kTexQB[3] = {0, 1, 0};

template <int TW, int NTO>
__device__ __forceinline__ void tex_load_a(u32x4 (&Ar)[TW], const u32x4* imgw, int s, int part, unsigned lane) {
  // explicit global address space: scalar base + 32-bit lane offset, no 64-bit per-lane address (gimg_t in mfma_split.h)
  typedef const __attribute__((address_space(1))) char* gbytes_t;
  const gbytes_t p = (gbytes_t)(imgw + (int64_t)s * (NTO * 2 * 64)) + part * 1024;
  const unsigned lane_off = lane * 16u;
#pragma unroll
  for (int t = 0; t < TW; ++t) Ar[t] = *(gimg_t)(p + t * 2048 + lane_off);
}

// BIAS: the first pass of a layer, acc = bias * (weight scale * the point tile's scale) (bias_h: K-order, wave-uniform)
template <int TW, int NB, int NTO, int KS, bool BIAS>
__device__ __forceinline__ void tex_gemm(const u32x4* imgw, int a_part, const u32x4* actl, int b_part, f32x16 (&acc)[TW][NB],
                                         int s0, u32x4 (&A)[4][TW], const u32x4* next_imgw, int next_s, int next_a_part,
                                         unsigned lane, const float* bias_h = nullptr, int w = 0, const float* zs = nullptr) {
  static_assert(KS % 4 == 0, "K-steps are processed in groups of four");
  constexpr int KAD = kTexAD;
  if constexpr (BIAS) {
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float* bp = bias_h + (2 * (TW * w + t) + p) * 16 + 8 * (lane >> 5);
        const f32x4 lo = *reinterpret_cast<const f32x4*>(bp);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(bp + 4);
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) { acc[t][n][8 * p + e] = lo[e] * zs[n]; acc[t][n][8 * p + 4 + e] = hi[e] * zs[n]; }
      }
  }
  u32x4 B[2][NB];
  auto ldB = [&](u32x4 (&Br)[NB], int s) {
    const u32x4* p = actl + s * (NB * kAP * 64) + b_part * 64;
#pragma unroll
    for (int n = 0; n < NB; ++n) Br[n] = p[n * kAP * 64];
  };
  ldB(B[0], s0);
  for (int i = 0; i < KS; i += 4) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int k = i + jj;
      if (k + KAD < KS) tex_load_a<TW, NTO>(A[(jj + KAD) & 3], imgw, s0 + k + KAD, a_part, lane);
      else tex_load_a<TW, NTO>(A[(jj + KAD) & 3], next_imgw, next_s + (k + KAD - KS), next_a_part, lane);
      if (k + 1 < KS) ldB(B[(jj + 1) & 1], s0 + k + 1);
      // the operand requests ride in the shadow of this K-step's MFMAs, as in gemm_x3
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int n = 0; n < NB; ++n)
          acc[t][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[jj][t]),
                                                             __builtin_bit_cast(f16x8, B[jj & 1][n]), acc[t][n], 0, 0, 0);
      constexpr int M = TW * NB;
#pragma unroll
      for (int g = 0; g < NB && g < M; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
#pragma unroll
      for (int g = 0; g < TW && g < M - NB; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      // (an operand set stays live until here: see x3_keep_alive in mfma_split.h)
#pragma unroll
      for (int t = 0; t < TW; ++t) asm volatile("" ::"v"(A[jj][t]));
#pragma unroll
      for (int n = 0; n < NB; ++n) asm volatile("" ::"v"(B[jj & 1][n]));
    }
  }
}

}  // namespace
