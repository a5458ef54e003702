// The chunked sums of the backward passes (grad_sums.h): the general dW partial on the f32 matrix instruction
// (idrgrad.hip; texgrad.hip and sirengrad.hip keep kernels of their own for their shapes) and the reduce over the partials
// (all three).
#include "grad_sums.h"
#include "mfma_split.h"

namespace {

// One wave per 64 x 64 tile of dW, both operands read row-major straight from the stashes (32 consecutive floats per half
// wave), two rows per matrix instruction in ascending order.  The 16-row groups go alternately on TWO accumulation chains,
// the last rows, fewer than sixteen, on the second, and the chains are added at the end -- a chain is half as long (with a
// single chain of 512 rows dW_1 of an eight-layer SIREN sat on the float64 margin).
__global__ __launch_bounds__(256) void k_grad_tn(GradTnArgs a) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int tiles_o = a.ldA / 64, tiles_i = a.ldB / 64;
  const int tile = blockIdx.x * 4 + w;
  if (tile >= tiles_o * tiles_i) return;             // no barrier below
  const int o0 = 64 * (tile / tiles_i), i0 = 64 * (tile % tiles_i);
  if (o0 >= a.out_rows || i0 >= a.out_cols) return;
  const int64_t ldA = a.ldA, ldB = a.ldB;
  const int64_t p0 = (int64_t)blockIdx.y * a.rows_per_chunk;
  const int64_t pend = p0 + a.rows_per_chunk < a.rows ? p0 + a.rows_per_chunk : a.rows;
  f32x16 acc[2][2][2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][t][u][r] = 0.f;
  const float* __restrict__ Ap = a.A + o0 + j;
  const float* __restrict__ Bp = a.B + i0 + j;
  auto group = [&](int64_t p, f32x16 (&ac)[2][2]) {      // sixteen rows: 32 loads in flight, then 32 matrix instructions
    float av[8][2], bv[8][2];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t pp = p + 2 * u + hh;
      av[u][0] = Ap[pp * ldA]; av[u][1] = Ap[pp * ldA + 32];
      bv[u][0] = Bp[pp * ldB]; bv[u][1] = Bp[pp * ldB + 32];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      ac[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], bv[u][0], ac[0][0], 0, 0, 0);
      ac[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], bv[u][1], ac[0][1], 0, 0, 0);
      ac[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], bv[u][0], ac[1][0], 0, 0, 0);
      ac[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], bv[u][1], ac[1][1], 0, 0, 0);
    }
  };
  int64_t p = p0;
  for (; p + 32 <= pend; p += 32) { group(p, acc[0]); group(p + 16, acc[1]); }
  if (p + 16 <= pend) { group(p, acc[0]); p += 16; }
  for (; p < pend; p += 2) {                   // the last rows, fewer than sixteen, on the second chain
    const int64_t pp = p + hh;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    if (pp < pend) {
      a0 = Ap[pp * ldA]; a1 = Ap[pp * ldA + 32];
      b0 = Bp[pp * ldB]; b1 = Bp[pp * ldB + 32];
    }
    acc[1][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[1][0][0], 0, 0, 0);
    acc[1][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1][0][1], 0, 0, 0);
    acc[1][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][1][0], 0, 0, 0);
    acc[1][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1][1], 0, 0, 0);
  }
  float* __restrict__ out = a.part + (int64_t)blockIdx.y * a.part_stride;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = i0 + 32 * u + j;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = o0 + 32 * t + 8 * (r >> 2) + 4 * hh + (r & 3);
        if (row < a.out_rows && col < a.out_cols) out[(int64_t)row * a.out_cols + col] = acc[0][t][u][r] + acc[1][t][u][r];
      }
    }
}

// one float64 chain per entry, one f32 rounding per workspace chunk
__global__ void k_grad_reduce(const float* __restrict__ part, int64_t part_stride, int n_part, int64_t count, int accumulate,
                              float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    double s = accumulate ? (double)out[i] : 0.0;
    for (int c = 0; c < n_part; ++c) s += (double)part[(int64_t)c * part_stride + i];
    out[i] = (float)s;
  }
}

}  // namespace

void grad_tn_launch(const GradTnArgs& a, int n_part, hipStream_t st) {
  const int tiles = (a.ldA / 64) * (a.ldB / 64);
  hipLaunchKernelGGL(k_grad_tn, dim3((tiles + 3) / 4, n_part), dim3(256), 0, st, a);
}

void grad_reduce_launch(const float* part, int64_t part_stride, int n_part, int64_t count, bool accumulate, float* out,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_grad_reduce, dim3(iso_stream_grid(count, 256)), dim3(256), 0, st, part, part_stride, n_part, count,
                     accumulate ? 1 : 0, out);
}
