// Per-point PCA of a K-nearest neighbourhood: estimate_pointcloud_local_coord_frames
// (DSS/utils/mathHelper.py:43-119).  The reference spends a (N,P,K,3) knn tensor, a batched SVD of (K,3) matrices
// (torch_batch_svd) and about ten torch ops on it; here one lane per query row gathers its K neighbours straight from
// `points` through the int64 kNN index, forms the neighbourhood mean and the centred 3x3 covariance, solves it with cyclic
// Jacobi in f32, sorts ascending and applies the reference's sign rule, all in registers.  The cloud means the sign rule
// needs come from a first launch of per-slice partial sums (fixed order, no atomics), so two runs are bit-identical.
#include "iso_common.h"
#include "pca_eig.h"

namespace {

constexpr int kMeanSlices = 64;        // partial sums per cloud of the cloud-mean pass (work: N * 64 * 3 doubles)
constexpr int kMeanBlock = 256;

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
    float l[3], v[3][3];
    pca_neighbourhood_eig(cloud, row, K, len, l, v);
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
