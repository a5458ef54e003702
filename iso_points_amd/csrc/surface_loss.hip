// The point-cloud regularisers of the splatting renderer: normal mollification, ProjectionLoss and RepulsionLoss
// (DSS/training/losses.py:149-515; include/isopoints.h section K has the formulas).
//
// One lane per neighbour slot, 32 lanes per row, two rows per wave.  A row's K indices are one coalesced 256-B read and
// its K distances one 128-B read; the neighbours' positions and normals are 12-B gathers out of L2 (the arrays are
// read-only, and the neighbours of one row lie next to each other).  Every sum over k is the same xor butterfly over the
// row's 32 lanes: a fixed order, the same bits in every lane, no atomics.  The reference's (N,P,K) and (N,P,K,3)
// temporaries (weights, gathered normals, differences) exist in registers only.
#include "iso_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SL_BLOCK = 256;           // 8 rows per workgroup
constexpr int SL_ROWS = SL_BLOCK / 32;

// sum over the 32 lanes of a row, in every one of them
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 load3(const float* __restrict__ a, int64_t row) {
  V3 v;
  v.x = a[row * 3]; v.y = a[row * 3 + 1]; v.z = a[row * 3 + 2];
  return v;
}

// F.normalize: v / max(|v|, 1e-12)
__device__ __forceinline__ V3 unit3(V3 v) {
  float n = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
  n = n > 1e-12f ? n : 1e-12f;
  V3 u;
  u.x = v.x / n; u.y = v.y / n; u.z = v.z / n;
  return u;
}

// exp(-|u(mj) - u(mi)|^2 inv_sigma2)
__device__ __forceinline__ float normal_w(V3 mj, V3 ui, float inv_sigma2) {
  const V3 uj = unit3(mj);
  const float dx = uj.x - ui.x, dy = uj.y - ui.y, dz = uj.z - ui.z;
  return expf(-((dx * dx + dy * dy) + dz * dz) * inv_sigma2);
}

// max(0, 1 - d / (((2 d0) fs) fs))^4
__device__ __forceinline__ float phi_w(float d, float d0, float fs) {
  const float s = ((d0 * 2.0f) * fs) * fs;
  float w = 1.0f - d / s;
  w = w < 0.f ? 0.f : w;
  w = w * w;
  return w * w;
}

// what every kernel here needs of its row: the slot's neighbour and distance, the nearest distance
struct Slot {
  int64_t j;      // neighbour row within the cloud; valid only when ok
  float d, d0;
  bool ok;
};

__device__ __forceinline__ Slot load_slot(const int64_t* __restrict__ idx, int64_t idx_stride,
                                          const float* __restrict__ dists, int64_t d_stride, int64_t row, int k, int K,
                                          int64_t p_stride) {
  Slot s;
  s.j = 0; s.d = 0.f; s.ok = false;
  if (k < K) {
    s.j = idx[row * idx_stride + k];
    s.d = dists[row * d_stride + k];
    s.ok = s.j >= 0 && s.j < p_stride;
    if (!s.ok) s.j = 0;
  }
  s.d0 = __shfl(s.d, 0, 32);
  return s;
}

__global__ __launch_bounds__(SL_BLOCK) void k_surfloss_mollify(
    const float* __restrict__ in, const int64_t* __restrict__ idx, int64_t idx_stride,
    const float* __restrict__ dists, int64_t d_stride, const int64_t* __restrict__ lengths, int64_t p_stride,
    int64_t n_rows, int K, float fs, float inv_sigma2, int use_normal_w, float* __restrict__ out) {
  const int k = threadIdx.x & 31;
  // n_rows is rounded up by the loop bound to whole workgroups so that every lane of a wave takes the same trips
  for (int64_t row = (int64_t)blockIdx.x * SL_ROWS + (threadIdx.x >> 5); row < n_rows;
       row += (int64_t)gridDim.x * SL_ROWS) {
    const int64_t n = row / p_stride, i = row - n * p_stride;
    const int64_t len = lengths ? lengths[n] : p_stride;
    if (i >= len) {
      if (k < 3) out[row * 3 + k] = 0.f;
      continue;
    }
    const Slot s = load_slot(idx, idx_stride, dists, d_stride, row, k, K, p_stride);
    const float* inn = in + n * p_stride * 3;
    V3 mj = {0.f, 0.f, 0.f};
    float w = 0.f;
    if (s.ok) {
      mj = load3(inn, s.j);
      w = phi_w(s.d, s.d0, fs);
      if (use_normal_w) w = w * normal_w(mj, unit3(load3(in, row)), inv_sigma2);
    }
    const float sw = row_sum(w);
    const float sx = row_sum(mj.x * w), sy = row_sum(mj.y * w), sz = row_sum(mj.z * w);
    const float den = iso_eps_denom(sw, 1.0e-17f);
    if (k == 0) {
      out[row * 3] = sx / den; out[row * 3 + 1] = sy / den; out[row * 3 + 2] = sz / den;
    }
  }
}

__global__ __launch_bounds__(SL_BLOCK) void k_surfloss_forward(
    const float* __restrict__ pts, const float* __restrict__ nbr_pts, const float* __restrict__ knn,
    const float* __restrict__ n1, const float* __restrict__ n2, const int64_t* __restrict__ idx, int64_t idx_stride,
    const float* __restrict__ dists, int64_t d_stride, const int64_t* __restrict__ lengths, int64_t p_stride,
    int64_t n_rows, int K, float fs, float inv_sigma2, int outputs, float* __restrict__ proj_out,
    float* __restrict__ rep_out, float* __restrict__ gproj_out, float* __restrict__ grep_out) {
  const int k = threadIdx.x & 31;
  const bool want_proj = outputs & ISO_SURFLOSS_PROJECTION, want_rep = outputs & ISO_SURFLOSS_REPULSION;
  const bool want_grad = outputs & ISO_SURFLOSS_GRADIENTS;
  for (int64_t row = (int64_t)blockIdx.x * SL_ROWS + (threadIdx.x >> 5); row < n_rows;
       row += (int64_t)gridDim.x * SL_ROWS) {
    const int64_t n = row / p_stride, i = row - n * p_stride;
    const int64_t len = lengths ? lengths[n] : p_stride;
    if (i >= len) {
      if (k == 0) {
        if (want_proj) proj_out[row] = 0.f;
        if (want_rep) rep_out[row] = 0.f;
      }
      if (k < 3 && want_grad) {
        if (want_proj) gproj_out[row * 3 + k] = 0.f;
        if (want_rep) grep_out[row * 3 + k] = 0.f;
      }
      continue;
    }
    const Slot s = load_slot(idx, idx_stride, dists, d_stride, row, k, K, p_stride);
    const V3 p = load3(pts, row);
    V3 x = p, m = {0.f, 0.f, 0.f};   // neighbour position and its n2; an empty slot sits on the point with weight 0
    float nu = 0.f, w = 0.f;
    bool ball = true;
    if (s.ok) {
      x = knn ? load3(knn, row * K + k) : load3(nbr_pts + n * p_stride * 3, s.j);
      m = load3(n2 + n * p_stride * 3, s.j);
      nu = normal_w(load3(n1 + n * p_stride * 3, s.j), unit3(load3(n1, row)), inv_sigma2);
      ball = s.d > (fs * s.d0) * 2.0f;
      w = ball ? 0.f : phi_w(s.d, s.d0, fs) * nu;
    }
    const float sk = ((x.x - p.x) * m.x + (x.y - p.y) * m.y) + (x.z - p.z) * m.z;
    const float den_w = iso_eps_denom(row_sum(w), 1.0e-17f);
    // sum_k w n2_j / sd(sum w): the projection's gradient direction and the tangent part of the repulsion's
    const float ax = row_sum(w * m.x) / den_w, ay = row_sum(w * m.y) / den_w, az = row_sum(w * m.z) / den_w;
    if (want_proj) {
      const float D = row_sum(w * sk) / den_w;
      if (k == 0) {
        proj_out[row] = D * D;
        if (want_grad) {
          const float c = 2.0f * D;
          gproj_out[row * 3] = c * -ax; gproj_out[row * 3 + 1] = c * -ay; gproj_out[row * 3 + 2] = c * -az;
        }
      }
    }
    if (!want_rep) continue;
    const float sw = sk * w;
    V3 q;
    q.x = p.x + row_sum(sw * m.x) / den_w;
    q.y = p.y + row_sum(sw * m.y) / den_w;
    q.z = p.z + row_sum(sw * m.z) / den_w;
    const float ex = q.x - x.x, ey = q.y - x.y, ez = q.z - x.z;
    const float e2 = (ex * ex + ey * ey) + ez * ez;
    const float sig = s.ok ? expf(-e2 * ((float)len * 0.5f)) : 0.f;
    const float dens = row_sum(sig) + 1.0f;
    const float W = ball ? 0.f : (nu * sig) * dens;
    const float den_W = iso_eps_denom(row_sum(W), 1.0e-17f);
    const float rep = -row_sum(e2 * W) / den_W;
    if (k == 0) rep_out[row] = rep;
    if (want_grad) {
      const float gx = -row_sum((2.0f * ex) * W) / den_W, gy = -row_sum((2.0f * ey) * W) / den_W,
                  gz = -row_sum((2.0f * ez) * W) / den_W;
      const float mg = w * ((m.x * gx + m.y * gy) + m.z * gz);
      const float bx = row_sum(mg * m.x) / den_w, by = row_sum(mg * m.y) / den_w, bz = row_sum(mg * m.z) / den_w;
      if (k == 0) {
        grep_out[row * 3] = gx - bx; grep_out[row * 3 + 1] = gy - by; grep_out[row * 3 + 2] = gz - bz;
      }
    }
  }
}

int surfloss_common(const char* who, const int64_t* idx, int64_t idx_stride, const float* dists, int64_t d_stride,
                    int n_clouds, int64_t p_stride, int K) {
  ISO_REQUIRE(K >= 1 && K <= 32, ISO_ERR_UNSUPPORTED, "%s: K must be in [1,32], got %d", who, K);
  ISO_REQUIRE(n_clouds >= 0 && p_stride >= 0, ISO_ERR_INVALID, "%s: bad sizes", who);
  ISO_REQUIRE(idx_stride >= K && d_stride >= K, ISO_ERR_INVALID, "%s: a row stride is smaller than K", who);
  ISO_REQUIRE((idx && dists) || n_clouds == 0 || p_stride == 0, ISO_ERR_INVALID, "%s: null pointer", who);
  return ISO_OK;
}

// every lane of a wave takes the same number of trips: the grid covers whole groups of SL_ROWS rows and the row test
// inside the loop is per 32-lane group, which the shuffles never leave
int surfloss_grid(int64_t n_rows) { return iso_stream_grid(n_rows, SL_ROWS); }

}  // namespace

extern "C" int iso_surfloss_mollify(const float* normals_in, const int64_t* idx, int64_t idx_row_stride,
                                    const float* dists, int64_t dists_row_stride, const int64_t* lengths, int n_clouds,
                                    int64_t p_stride, int K, float filter_scale, float inv_sigma2,
                                    int use_normal_w, float* normals_out, void* stream) {
  int rc = surfloss_common("iso_surfloss_mollify", idx, idx_row_stride, dists, dists_row_stride, n_clouds, p_stride, K);
  if (rc != ISO_OK) return rc;
  if (n_clouds == 0 || p_stride == 0) return ISO_OK;
  ISO_REQUIRE(normals_in && normals_out, ISO_ERR_INVALID, "iso_surfloss_mollify: null pointer");
  ISO_REQUIRE(normals_in != normals_out, ISO_ERR_INVALID, "iso_surfloss_mollify: in-place not allowed (neighbours are re-read)");
  const int64_t n_rows = (int64_t)n_clouds * p_stride;
  hipLaunchKernelGGL(k_surfloss_mollify, dim3(surfloss_grid(n_rows)), dim3(SL_BLOCK), 0, (hipStream_t)stream, normals_in,
                     idx, idx_row_stride, dists, dists_row_stride, lengths, p_stride, n_rows, K, filter_scale,
                     inv_sigma2, use_normal_w, normals_out);
  ISO_CHECK_LAUNCH("iso_surfloss_mollify");
  return ISO_OK;
}

extern "C" int iso_surfloss_forward(const float* points, const float* nbr_points, const float* knn, const float* n1,
                                    const float* n2, const int64_t* idx, int64_t idx_row_stride, const float* dists,
                                    int64_t dists_row_stride, const int64_t* lengths, int n_clouds, int64_t p_stride, int K, float filter_scale, float inv_sigma2, int outputs,
                                    float* proj_out, float* rep_out, float* grad_proj_out, float* grad_rep_out,
                                    void* stream) {
  int rc = surfloss_common("iso_surfloss_forward", idx, idx_row_stride, dists, dists_row_stride, n_clouds, p_stride, K);
  if (rc != ISO_OK) return rc;
  const int all = ISO_SURFLOSS_PROJECTION | ISO_SURFLOSS_REPULSION | ISO_SURFLOSS_GRADIENTS;
  ISO_REQUIRE((outputs & ~all) == 0 && (outputs & (ISO_SURFLOSS_PROJECTION | ISO_SURFLOSS_REPULSION)) != 0,
              ISO_ERR_INVALID, "iso_surfloss_forward: outputs must name the projection, the repulsion or both, got %d",
              outputs);
  if (n_clouds == 0 || p_stride == 0) return ISO_OK;
  const bool grad = outputs & ISO_SURFLOSS_GRADIENTS;
  ISO_REQUIRE(points && (nbr_points || knn) && n1 && n2, ISO_ERR_INVALID, "iso_surfloss_forward: null pointer");
  ISO_REQUIRE(!(outputs & ISO_SURFLOSS_PROJECTION) || (proj_out && (!grad || grad_proj_out)), ISO_ERR_INVALID,
              "iso_surfloss_forward: the projection is asked for without its output arrays");
  ISO_REQUIRE(!(outputs & ISO_SURFLOSS_REPULSION) || (rep_out && (!grad || grad_rep_out)), ISO_ERR_INVALID,
              "iso_surfloss_forward: the repulsion is asked for without its output arrays");
  const int64_t n_rows = (int64_t)n_clouds * p_stride;
  hipLaunchKernelGGL(k_surfloss_forward, dim3(surfloss_grid(n_rows)), dim3(SL_BLOCK), 0, (hipStream_t)stream, points,
                     nbr_points, knn, n1, n2, idx, idx_row_stride, dists, dists_row_stride, lengths, p_stride,
                     n_rows, K, filter_scale, inv_sigma2, outputs, proj_out, rep_out, grad_proj_out, grad_rep_out);
  ISO_CHECK_LAUNCH("iso_surfloss_forward");
  return ISO_OK;
}
