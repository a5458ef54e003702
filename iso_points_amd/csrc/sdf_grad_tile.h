// What the two SDF backward sweeps share (k_sirengrad_sweep of sirengrad.hip, k_idrgrad_sweep of idrgrad.hip; DESIGN.md
// 3.1e).  The tile is 4 waves x 16 matrix-instruction columns, a column being a point or, in the tangent form, the value
// (lane j < 8) or tangent (lane j + 8) half of a point; NT * 256 floats of LDS per wave hold the columns' H = 16 NT
// features as hL4[e4 * 64 + lane] = features 16 e4 + 4 g .. + 3.
#pragma once
#include "mlp_common.h"

// one reverse layer: the adjoints in LDS times the transposed image BW, back into LDS
template <int NT>
__device__ __forceinline__ void sdf_grad_reverse_gemm(const float* BW, float* hL, float* wbuf, f32x4 (&acc)[NT], int lane, int g) {
  gemm_pass<NT, false>(BW, nullptr, hL, wbuf, acc, lane, g);
  f32x4* hL4 = reinterpret_cast<f32x4*>(hL);
#pragma unroll
  for (int t = 0; t < NT; ++t) hL4[t * 64 + lane] = acc[t];
}

// dx of a point: the float64 partial sums of its lanes (four g, and the tangent lane where XOR8) added, rounded once, stored
template <bool XOR8>
__device__ __forceinline__ void sdf_grad_store_dx(double gx, double gy, double gz, float* dx, int64_t p, bool store) {
  gx += __shfl_xor(gx, 16); gx += __shfl_xor(gx, 32);
  gy += __shfl_xor(gy, 16); gy += __shfl_xor(gy, 32);
  gz += __shfl_xor(gz, 16); gz += __shfl_xor(gz, 32);
  if constexpr (XOR8) { gx += __shfl_xor(gx, 8); gy += __shfl_xor(gy, 8); gz += __shfl_xor(gz, 8); }
  if (store) { dx[p * 3] = (float)gx; dx[p * 3 + 1] = (float)gy; dx[p * 3 + 2] = (float)gz; }
}
