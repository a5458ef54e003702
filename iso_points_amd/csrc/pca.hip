// Per-point PCA of a K-nearest neighbourhood: estimate_pointcloud_local_coord_frames
// (DSS/utils/mathHelper.py:43-119).  The reference spends a (N,P,K,3) knn tensor, a batched SVD of (K,3) matrices
// (torch_batch_svd) and about ten torch ops on it; here one lane per query row gathers its K neighbours straight from
// `points` through the int64 kNN index, forms the neighbourhood mean and the centred 3x3 covariance, solves it with cyclic
// Jacobi in f32, sorts ascending and applies the reference's sign rule, all in registers.  The cloud means the sign rule
// needs come from a first launch of per-slice partial sums (fixed order, no atomics), so two runs are bit-identical.
#include "iso_common.h"

namespace {

constexpr int kMeanSlices = 64;        // partial sums per cloud of the cloud-mean pass (work: N * 64 * 3 doubles)
constexpr int kMeanBlock = 256;
// Cyclic Jacobi on a 3x3 symmetric matrix converges quadratically once the off-diagonal part is below the eigenvalue gaps:
// from a generic start the off-diagonal norm goes ~1 -> 1e-1 -> 1e-2 -> 1e-4 -> 1e-8 relative, i.e. below f32 rounding after
// four sweeps.  Near-degenerate spectra (edges and corners of a cube, collinear runs) converge linearly for the first sweep
// or two before the quadratic phase, so two more sweeps are kept; once an off-diagonal entry is exactly zero a rotation is the
// identity (t = 0 by select, below), so extra sweeps cost 3 x ~30 VALU instructions and change nothing.  The count is a
// compile-time constant, hence wave-uniform: no lane waits on another's convergence test.
constexpr int kJacobiSweeps = 6;

// Cloud sums over the first lengths[b] rows: workgroup (s, b) adds slice s of cloud b in double, then a fixed-shape
// tree in LDS; one double3 per (b, s).
__global__ void k_pca_cloud_sums(const float* __restrict__ pts, const int64_t* __restrict__ lengths, int64_t P,
                                 double* __restrict__ part) {
  __shared__ double s_sum[3][kMeanBlock];
  const int b = blockIdx.y, s = blockIdx.x;
  const int64_t len = lengths ? min(max(lengths[b], (int64_t)0), P) : P;
  const int64_t chunk = (len + kMeanSlices - 1) / kMeanSlices;
  const int64_t lo = s * chunk, hi = min(lo + chunk, len);
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kMeanBlock) {
    const float* p = pts + ((int64_t)b * P + i) * 3;
    ax += (double)p[0];
    ay += (double)p[1];
    az += (double)p[2];
  }
  s_sum[0][threadIdx.x] = ax;
  s_sum[1][threadIdx.x] = ay;
  s_sum[2][threadIdx.x] = az;
  __syncthreads();
  for (int w = kMeanBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      s_sum[0][threadIdx.x] += s_sum[0][threadIdx.x + w];
      s_sum[1][threadIdx.x] += s_sum[1][threadIdx.x + w];
      s_sum[2][threadIdx.x] += s_sum[2][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) part[((int64_t)b * kMeanSlices + s) * 3 + threadIdx.x] = s_sum[threadIdx.x][0];
}

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

// One lane per query row (b, i); workgroup column b = cloud.  mu: per-cloud partial sums (disambiguate only).
__global__ void __launch_bounds__(256) k_pca_frames(const float* __restrict__ pts, const int64_t* __restrict__ lengths,
                                                    const int64_t* __restrict__ idx, int64_t P, int K, int disambiguate,
                                                    const double* __restrict__ part, float* __restrict__ curv,
                                                    float* __restrict__ frames) {
  __shared__ float s_mu[3];
  const int b = blockIdx.y;
  const int64_t len = lengths ? min(max(lengths[b], (int64_t)0), P) : P;
  if (disambiguate) {
    if (threadIdx.x < 3) {
      double acc = 0.0;
      for (int s = 0; s < kMeanSlices; ++s) acc += part[((int64_t)b * kMeanSlices + s) * 3 + threadIdx.x];
      s_mu[threadIdx.x] = (float)(acc / (double)(len > 0 ? len : 1));
    }
    __syncthreads();
  }
  const float* cloud = pts + (int64_t)b * P * 3;
  const float inv_k = 1.0f / (float)K;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = (int64_t)b * P + i;
    float* co = curv + g * 3;
    float* fo = frames + g * 9;
    if (i >= len) {
#pragma unroll
      for (int k = 0; k < 3; ++k) co[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 9; ++k) fo[k] = 0.0f;
      continue;
    }
    const int64_t* row = idx + g * K;
    // pass 1: neighbourhood mean (pt_mean, :84), accumulated relative to the first neighbour: the sums stay small next to
    // the coordinates (a cloud far from the origin loses no bits to them), and K exact duplicates give m = x_0 exactly, so
    // their covariance is exactly 0 (remove_outliers then sees the reference's 0 / 0).  An index outside [0, len) is
    // clamped into the cloud: kNN never returns one for a valid row of a cloud longer than K, and the clamp keeps every
    // read inside the points tensor.
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
    const float mx = ox + sx * inv_k, my = oy + sy * inv_k, mz = oz + sz * inv_k;
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
    float v[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
#pragma unroll
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate<0, 1, 2>(a, v);
      jacobi_rotate<0, 2, 1>(a, v);
      jacobi_rotate<1, 2, 0>(a, v);
    }
    // eigenvalues = S^2 / K of the reference's SVD (:93-94), clamped at 0, ascending (:99-100)
    float l[3] = {fmaxf(a[0][0], 0.0f), fmaxf(a[1][1], 0.0f), fmaxf(a[2][2], 0.0f)};
    order_pair<0, 1>(l, v);
    order_pair<1, 2>(l, v);
    order_pair<0, 1>(l, v);
    if (disambiguate) {
      // _disambiguate_vector_directions(points_centered, knn, v) for v = column 0 (n) and column 2 (z) (:105-113): the
      // test vectors are d_j = x_j - (p_i - mu_b), the uncentred neighbours against the GLOBALLY centred point; a direction
      // flips when fewer than K/2 of its projections are positive.  Then y = n x z and the frame is (n, y, z).
      const float* p = cloud + i * 3;
      const float cx = p[0] - s_mu[0], cy = p[1] - s_mu[1], cz = p[2] - s_mu[2];
      int pos_n = 0, pos_z = 0;
  #pragma unroll 4
    for (int j = 0; j < K; ++j) {
        const int64_t n = min(max(row[j], (int64_t)0), len - 1);
        const float* x = cloud + n * 3;
        const float dx = x[0] - cx, dy = x[1] - cy, dz = x[2] - cz;
        pos_n += ((v[0][0] * dx + v[1][0] * dy) + v[2][0] * dz) > 0.0f ? 1 : 0;
        pos_z += ((v[0][2] * dx + v[1][2] * dy) + v[2][2] * dz) > 0.0f ? 1 : 0;
      }
      const float fn = (2 * pos_n < K) ? -1.0f : 1.0f;
      const float fz = (2 * pos_z < K) ? -1.0f : 1.0f;
      const float n0 = fn * v[0][0], n1 = fn * v[1][0], n2 = fn * v[2][0];
      const float z0 = fz * v[0][2], z1 = fz * v[1][2], z2 = fz * v[2][2];
      v[0][0] = n0; v[1][0] = n1; v[2][0] = n2;
      v[0][2] = z0; v[1][2] = z1; v[2][2] = z2;
      v[0][1] = n1 * z2 - n2 * z1;
      v[1][1] = n2 * z0 - n0 * z2;
      v[2][1] = n0 * z1 - n1 * z0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) co[k] = l[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) fo[r * 3 + c] = v[r][c];
  }
}

}  // namespace

extern "C" int64_t iso_pca_frames_work_bytes(int n_clouds) {
  return n_clouds > 0 ? (int64_t)n_clouds * kMeanSlices * 3 * (int64_t)sizeof(double) : 0;
}

extern "C" int iso_pca_frames(const float* points, const int64_t* lengths, const int64_t* idx, int n_clouds,
                              int64_t max_points, int K, int disambiguate, void* work, float* curvature_out,
                              float* frames_out, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && max_points >= 0 && K >= 1, ISO_ERR_INVALID, "iso_pca_frames: bad sizes");
  if (n_clouds == 0 || max_points == 0) return ISO_OK;
  ISO_REQUIRE(points && idx && curvature_out && frames_out, ISO_ERR_INVALID, "iso_pca_frames: null pointer");
  ISO_REQUIRE(!disambiguate || work, ISO_ERR_INVALID, "iso_pca_frames: disambiguate needs the work buffer");
  hipStream_t s = (hipStream_t)stream;
  if (disambiguate) {
    hipLaunchKernelGGL(k_pca_cloud_sums, dim3(kMeanSlices, n_clouds), dim3(kMeanBlock), 0, s, points, lengths, max_points,
                       (double*)work);
    ISO_CHECK_LAUNCH("iso_pca_frames (cloud sums)");
  }
  hipLaunchKernelGGL(k_pca_frames, dim3(iso_stream_grid(max_points, 256), n_clouds), dim3(256), 0, s, points, lengths, idx,
                     max_points, K, disambiguate ? 1 : 0, (const double*)work, curvature_out, frames_out);
  ISO_CHECK_LAUNCH("iso_pca_frames");
  return ISO_OK;
}
