// The planned reduction of the three backward passes (texgrad.hip, sirengrad.hip, idrgrad.hip): a weight
// gradient is a sum over the points, cut into FIXED chunks of points so that its bits do not depend on the grid --
//   dW_l = A^T B per chunk on the f32 32x32x2 matrix instruction, the general form (a row length per operand, the true
//             size of the matrix); texgrad.hip (one chain, 512-point chunks) and sirengrad.hip (square layers) keep
//             kernels of their own, which measured faster on their shapes             k_grad_tn
//   the column sums (biases, heads) per chunk in float64: they index each family's own raw layout and stay in its file;
//             a workgroup takes a chunk in four quarters                                                grad_quarter_range
//   the partials added in chunk order, on top of the earlier workspace chunks                           k_grad_reduce
// The kernels are in grad_sums.hip; no float atomic anywhere.
#pragma once
#include "iso_common.h"

// part[c][o][i] = sum over the rows r of chunk c of A[r][o] B[r][i].  One wave per 64 x 64 tile of the (ldA, ldB) product;
// rows at or past out_rows and columns at or past out_cols (a narrow layer, an operand's padding) are not written.
struct GradTnArgs {
  const float* A;                    // adjoint rows (rows, ldA)
  const float* B;                    // input rows (rows, ldB)
  int ldA, ldB;                      // multiples of 64
  int64_t rows;
  int64_t rows_per_chunk;
  float* part;                       // partial c at part + c * part_stride, row-major (out_rows, out_cols)
  int64_t part_stride;
  int out_rows, out_cols;
};

// two accumulation chains over a chunk's rows; grid (ceil(tiles / 4), n_part)
void grad_tn_launch(const GradTnArgs& a, int n_part, hipStream_t st);

// out[i] = (accumulate ? out[i] : 0) + part[0][i] + .. + part[n_part - 1][i], i < count
void grad_reduce_launch(const float* part, int64_t part_stride, int n_part, int64_t count, bool accumulate, float* out,
                        hipStream_t st);

// [p0, pend): quarter q of chunk `chunk` (part_points points each) of m points; empty past the end
__device__ __forceinline__ void grad_quarter_range(int chunk, int q, int part_points, int64_t m, int64_t& p0, int64_t& pend) {
  const int64_t c0 = (int64_t)chunk * part_points;
  const int64_t cend = c0 + part_points < m ? c0 + part_points : m;
  const int quarter = part_points / 4;
  p0 = c0 + (int64_t)q * quarter;
  pend = p0 + quarter < cend ? p0 + quarter : cend;
  if (p0 > pend) p0 = pend;
}
