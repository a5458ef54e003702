// Eigen-decomposition of a K-neighbourhood's covariance, in registers: the device code that the local-frame kernel
// (pca.hip, k_pca_frames) and the fused anisotropic splat set-up (splat.hip, k_splat_setup_aniso) share, so that the two
// produce the same bits from the same neighbours.
#pragma once
#include "iso_common.h"

#pragma clang fp contract(off)

namespace {

// Cyclic Jacobi on a 3x3 symmetric matrix converges quadratically once the off-diagonal part is below the eigenvalue gaps:
// from a generic start the off-diagonal norm goes ~1 -> 1e-1 -> 1e-2 -> 1e-4 -> 1e-8 relative, i.e. below f32 rounding after
// four sweeps.  Near-degenerate spectra (edges and corners of a cube, collinear runs) converge linearly for the first sweep
// or two before the quadratic phase, so two more sweeps are kept; once an off-diagonal entry is exactly zero a rotation is the
// identity (t = 0 by select, below), so extra sweeps cost 3 x ~30 VALU instructions and change nothing.  The count is a
// compile-time constant, hence wave-uniform: no lane waits on another's convergence test.
constexpr int kJacobiSweeps = 6;

// One Jacobi rotation in the (p, q) plane (Numerical Recipes' jacobi, Golub & Van Loan's sym.schur2): t = tan of the angle
// that zeroes a_pq, picked as the smaller root; a_pq == 0 gives t = 0 (identity) by select.  a is the symmetric matrix
// (upper triangle used), v accumulates the eigenvectors as columns.
template <int p, int q, int r>
__device__ __forceinline__ void jacobi_rotate(float (&a)[3][3], float (&v)[3][3]) {
  const float apq = a[p][q];
  const float tau = (a[q][q] - a[p][p]) / (2.0f * apq);
  const float tt = copysignf(1.0f, tau) / (fabsf(tau) + sqrtf(1.0f + tau * tau));
  const float t = (apq != 0.0f && tt == tt) ? tt : 0.0f;
  const float c = 1.0f / sqrtf(1.0f + t * t);
  const float s = t * c;
  a[p][p] = a[p][p] - t * apq;
  a[q][q] = a[q][q] + t * apq;
  a[p][q] = 0.0f;
  // the third row / column (r != p, q), stored at (min, max)
  const float arp = (r < p) ? a[r][p] : a[p][r];
  const float arq = (r < q) ? a[r][q] : a[q][r];
  const float nrp = c * arp - s * arq;
  const float nrq = s * arp + c * arq;
  if (r < p) a[r][p] = nrp; else a[p][r] = nrp;
  if (r < q) a[r][q] = nrq; else a[q][r] = nrq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float vp = v[k][p], vq = v[k][q];
    v[k][p] = c * vp - s * vq;
    v[k][q] = s * vp + c * vq;
  }
}

// Compare-exchange of eigenpairs i < j by selects (no conditional swap block: DESIGN.md 7, item 6).
template <int i, int j>
__device__ __forceinline__ void order_pair(float (&l)[3], float (&v)[3][3]) {
  const bool sw = l[i] > l[j];
  const float li = l[i], lj = l[j];
  l[i] = sw ? lj : li;
  l[j] = sw ? li : lj;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float vi = v[k][i], vj = v[k][j];
    v[k][i] = sw ? vj : vi;
    v[k][j] = sw ? vi : vj;
  }
}

// Neighbourhood mean (pt_mean, :84), accumulated relative to the first neighbour: the sums stay small next to the
// coordinates (a cloud far from the origin loses no bits to them), and K exact duplicates give m = x_0 exactly, so their
// covariance is exactly 0 (remove_outliers then sees the reference's 0 / 0).  An index outside [0, len) is clamped into
// the cloud: kNN never returns one for a valid row of a cloud longer than K, and the clamp keeps every read inside the
// points tensor.  The backward pass (pca_backward.hip) centres on the same bits.
__device__ __forceinline__ void pca_neighbourhood_mean(const float* __restrict__ cloud, const int64_t* __restrict__ row, int K,
                                                       int64_t len, float inv_k, float& mx, float& my, float& mz) {
  const float* x0 = cloud + min(max(row[0], (int64_t)0), len - 1) * 3;
  const float ox = x0[0], oy = x0[1], oz = x0[2];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll 4
  for (int j = 0; j < K; ++j) {
    const int64_t n = min(max(row[j], (int64_t)0), len - 1);
    const float* x = cloud + n * 3;
    sx += x[0] - ox;
    sy += x[1] - oy;
    sz += x[2] - oz;
  }
  mx = ox + sx * inv_k;
  my = oy + sy * inv_k;
  mz = oz + sz * inv_k;
}

// Neighbourhood mean, centred covariance (1/K) sum (x_j - m)(x_j - m)^T, cyclic Jacobi, eigenvalues clamped at 0 and sorted
// ascending with their eigenvectors (column c of v belongs to l[c]; signs as Jacobi leaves them).  cloud: the cloud's
// first point; row: the K neighbour indices of the query (the point itself included); len: points in the cloud.
__device__ __forceinline__ void pca_neighbourhood_eig(const float* __restrict__ cloud, const int64_t* __restrict__ row, int K,
                                                      int64_t len, float (&l)[3], float (&v)[3][3]) {
  const float inv_k = 1.0f / (float)K;
  // pass 1: the mean
  float mx, my, mz;
  pca_neighbourhood_mean(cloud, row, K, len, inv_k, mx, my, mz);
  // pass 2: centred products (central_diff, :87); the second read of the K neighbours hits cache
  float cxx = 0.0f, cxy = 0.0f, cxz = 0.0f, cyy = 0.0f, cyz = 0.0f, czz = 0.0f;
#pragma unroll 4
  for (int j = 0; j < K; ++j) {
    const int64_t n = min(max(row[j], (int64_t)0), len - 1);
    const float* x = cloud + n * 3;
    const float dx = x[0] - mx, dy = x[1] - my, dz = x[2] - mz;
    cxx += dx * dx;
    cxy += dx * dy;
    cxz += dx * dz;
    cyy += dy * dy;
    cyz += dy * dz;
    czz += dz * dz;
  }
  float a[3][3] = {{cxx * inv_k, cxy * inv_k, cxz * inv_k}, {0.0f, cyy * inv_k, cyz * inv_k}, {0.0f, 0.0f, czz * inv_k}};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0f : 0.0f;
#pragma unroll
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate<0, 1, 2>(a, v);
    jacobi_rotate<0, 2, 1>(a, v);
    jacobi_rotate<1, 2, 0>(a, v);
  }
  // eigenvalues = S^2 / K of the reference's SVD (:93-94), clamped at 0, ascending (:99-100)
  l[0] = fmaxf(a[0][0], 0.0f);
  l[1] = fmaxf(a[1][1], 0.0f);
  l[2] = fmaxf(a[2][2], 0.0f);
  order_pair<0, 1>(l, v);
  order_pair<1, 2>(l, v);
  order_pair<0, 1>(l, v);
}

}  // namespace
