// Backward pass of the local-frame estimator (pca.hip; DSS/utils/mathHelper.py:43-119 under autograd, which the reference
// gets from torch_batch_svd's backward).  With the neighbour index, the ascending order, the clamp and the two sign factors
// of the forward held constant, the forward is m = mean x_j, C = (1/K) sum (x_j - m)(x_j - m)^T = V diag(l) V^T and the
// gradient w.r.t. the points is a sum over the slots (i, j) that hold a point:
//   grad[t] = sum_{(i,j): idx[i,j] = t} (2/K) G_i (x_t - m_i),   G_i = V (diag(g_l) + S) V^T,
//   S_ab = (v_a.gv_b - v_b.gv_a) / (2 (l_b - l_a)).
// k_pca_adjoint (one lane per query row) reads the forward's own outputs and writes G_i, m_i and the row's K targets as
// int32; gather_lists.h sorts the P*K slots by target (integer atomics only); k_pca_scatter sums every target's list in
// ascending slot order.  No float atomics: two runs give the same bits.
#include "iso_common.h"
#include "pca_eig.h"
#include "gather_lists.h"

namespace {

constexpr int kAdjFloats = 9;       // per query row: G (xx, xy, xz, yy, yz, zz) and m
constexpr int kLaneList = 64;       // a target in at most this many slots sorts and sums its list in its own lane; the mean
                                    // list holds K <= 32 slots (the in-degree of a kNN graph), so that is nearly every target
constexpr float kGapTol = 2e-5f;    // eigenvalue pairs closer than this times l_max exchange nothing: the forward's own
                                    // eigenvalue tolerance, below which the sign of the gap is not determined

// S_ab of the symmetric eigen adjoint for the pair (a, b); 0 by select where the gap is within tol (a NaN or an infinity of
// the quotient never leaves the select)
template <int a, int b>
__device__ __forceinline__ float pair_adjoint(const float (&l)[3], const float (&v)[3][3], const float (&gv)[3][3], float tol) {
  const float m_ab = (v[0][a] * gv[0][b] + v[1][a] * gv[1][b]) + v[2][a] * gv[2][b];
  const float m_ba = (v[0][b] * gv[0][a] + v[1][b] * gv[1][a]) + v[2][b] * gv[2][a];
  const float gap = l[b] - l[a];
  const float s = (m_ab - m_ba) / (2.0f * gap);
  return fabsf(gap) > tol ? s : 0.0f;
}

// One lane per query row (b, i), laid out like k_pca_frames.  Rows i >= lengths[b] write K targets of -1 and nothing else:
// no list ever names them, so whatever the incoming gradients hold there is never read.
__global__ void __launch_bounds__(256) k_pca_adjoint(const float* __restrict__ pts, const int64_t* __restrict__ lengths,
                                                     const int64_t* __restrict__ idx, int64_t P, int K, int disambiguate,
                                                     const float* __restrict__ curv, const float* __restrict__ frames,
                                                     const float* __restrict__ g_curv, const float* __restrict__ g_frames,
                                                     float* __restrict__ adj, int32_t* __restrict__ flat) {
  const int b = blockIdx.y;
  const int64_t len = lengths ? min(max(lengths[b], (int64_t)0), P) : P;
  const float* cloud = pts + (int64_t)b * P * 3;
  const float inv_k = 1.0f / (float)K;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = (int64_t)b * P + i;
    const int64_t* row = idx + g * K;
    int32_t* fl = flat + g * K;
    if (i >= len) {
      for (int j = 0; j < K; ++j) fl[j] = -1;
      continue;
    }
    // the slot's target, clamped as the forward clamps it
    for (int j = 0; j < K; ++j) fl[j] = (int32_t)min(max(row[j], (int64_t)0), len - 1);
    float mx, my, mz;
    pca_neighbourhood_mean(cloud, row, K, len, inv_k, mx, my, mz);
    float l[3], gl[3], v[3][3], gf[3][3], gv[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      l[c] = curv[g * 3 + c];
      gl[c] = g_curv ? g_curv[g * 3 + c] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[r][c] = frames[g * 9 + r * 3 + c];
        gf[r][c] = g_frames ? g_frames[g * 9 + r * 3 + c] : 0.0f;
      }
    if (disambiguate) {
      // frames = (n, n x z, z) with n = fn v_0, z = fz v_2: gn = g_0 + z x g_1, gz = g_2 + g_1 x n.  G is even in every
      // column's sign, so the saved (n, y, z) with (gn, 0, gz) stand for (v_0, v_1, v_2) with (fn gn, 0, fz gz).
      gv[0][0] = gf[0][0] + (v[1][2] * gf[2][1] - v[2][2] * gf[1][1]);
      gv[1][0] = gf[1][0] + (v[2][2] * gf[0][1] - v[0][2] * gf[2][1]);
      gv[2][0] = gf[2][0] + (v[0][2] * gf[1][1] - v[1][2] * gf[0][1]);
      gv[0][2] = gf[0][2] + (gf[1][1] * v[2][0] - gf[2][1] * v[1][0]);
      gv[1][2] = gf[1][2] + (gf[2][1] * v[0][0] - gf[0][1] * v[2][0]);
      gv[2][2] = gf[2][2] + (gf[0][1] * v[1][0] - gf[1][1] * v[0][0]);
      gv[0][1] = 0.0f; gv[1][1] = 0.0f; gv[2][1] = 0.0f;
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) gv[r][c] = gf[r][c];
    }
    const float tol = kGapTol * fmaxf(fmaxf(l[0], l[1]), l[2]);
    const float s01 = pair_adjoint<0, 1>(l, v, gv, tol);
    const float s02 = pair_adjoint<0, 2>(l, v, gv, tol);
    const float s12 = pair_adjoint<1, 2>(l, v, gv, tol);
    // an eigenvalue that is 0 in the forward's output passes nothing: it was clamped, or it is exactly 0 and every d_ij is
    // orthogonal to its direction
    const float d0 = l[0] > 0.0f ? gl[0] : 0.0f, d1 = l[1] > 0.0f ? gl[1] : 0.0f, d2 = l[2] > 0.0f ? gl[2] : 0.0f;
    // G = V (diag(d) + S) V^T, S symmetric: row r of W = V (diag(d) + S), then G_rs = W_r . V_s
    float w[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      w[r][0] = (v[r][0] * d0 + v[r][1] * s01) + v[r][2] * s02;
      w[r][1] = (v[r][0] * s01 + v[r][1] * d1) + v[r][2] * s12;
      w[r][2] = (v[r][0] * s02 + v[r][1] * s12) + v[r][2] * d2;
    }
    float* a = adj + g * kAdjFloats;
    a[0] = (w[0][0] * v[0][0] + w[0][1] * v[0][1]) + w[0][2] * v[0][2];
    a[1] = (w[0][0] * v[1][0] + w[0][1] * v[1][1]) + w[0][2] * v[1][2];
    a[2] = (w[0][0] * v[2][0] + w[0][1] * v[2][1]) + w[0][2] * v[2][2];
    a[3] = (w[1][0] * v[1][0] + w[1][1] * v[1][1]) + w[1][2] * v[1][2];
    a[4] = (w[1][0] * v[2][0] + w[1][1] * v[2][1]) + w[1][2] * v[2][2];
    a[5] = (w[2][0] * v[2][0] + w[2][1] * v[2][1]) + w[2][2] * v[2][2];
    a[6] = mx; a[7] = my; a[8] = mz;
  }
}

struct PcaScatter {
  const float* pts;
  const int64_t* lengths;
  const float* adj;
  GatherView lists;          // queries = the P*K slots of a cloud, targets = its P points
  int32_t* heavy;
  int32_t* heavy_count;
  float* grad;
  int64_t P;
  int K;
};

// acc += G_i (x - m_i) for slot q = i * K + j of the cloud whose adjoint rows start at `adj`
__device__ __forceinline__ void add_slot(const float* __restrict__ adj, int K, int q, const float (&x)[3], float (&acc)[3]) {
  const float* a = adj + (int64_t)(q / K) * kAdjFloats;
  const float dx = x[0] - a[6], dy = x[1] - a[7], dz = x[2] - a[8];
  acc[0] += (a[0] * dx + a[1] * dy) + a[2] * dz;
  acc[1] += (a[1] * dx + a[3] * dy) + a[4] * dz;
  acc[2] += (a[2] * dx + a[4] * dy) + a[5] * dz;
}

// One lane per target point: its list (arrival order) is insertion-sorted in place -- the segment is the lane's own -- and
// summed in ascending slot order.  A list longer than kLaneList is left to k_pca_scatter_heavy (this kernel writes 0).
__global__ void __launch_bounds__(256) k_pca_scatter(PcaScatter s) {
  const int n = blockIdx.y;
  const int64_t len = s.lengths ? min(max(s.lengths[n], (int64_t)0), s.P) : s.P;
  const float* adj = s.adj + (int64_t)n * s.P * kAdjFloats;
  const float scale = 2.0f / (float)s.K;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.P; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = (int64_t)n * s.P + i;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (i < len) {
      const int L = s.lists.cnt[(int64_t)n * s.lists.t_stride + i];
      if (L > kLaneList) {
        s.heavy[atomicAdd(s.heavy_count, 1)] = (int32_t)r;   // the order of this list decides nothing: one wave per entry
      } else if (L > 0) {
        int32_t* li = s.lists.list + (int64_t)n * s.lists.q_stride + s.lists.off[(int64_t)n * s.lists.t_stride + i];
        for (int m = 1; m < L; ++m) {
          const int32_t q = li[m];
          int k = m - 1;
          while (k >= 0 && li[k] > q) { li[k + 1] = li[k]; --k; }
          li[k + 1] = q;
        }
        const float x[3] = {s.pts[r * 3 + 0], s.pts[r * 3 + 1], s.pts[r * 3 + 2]};
        for (int m = 0; m < L; ++m) add_slot(adj, s.K, li[m], x, acc);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s.grad[r * 3 + c] = scale * acc[c];
  }
}

// One wave per long list (gather_wave): every lane's sum runs in ascending slot order and the 64 sums are added by one
// butterfly, a fixed order.
__global__ void __launch_bounds__(64) k_pca_scatter_heavy(PcaScatter s) {
  __shared__ int32_t s_raw[kSortList], s_sorted[kSortList];
  const int lane = threadIdx.x;
  const int count = *s.heavy_count;
  const float scale = 2.0f / (float)s.K;
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int64_t r = s.heavy[w];
    const int n = (int)(r / s.P);
    const int i = (int)(r - (int64_t)n * s.P);
    const int L = s.lists.cnt[(int64_t)n * s.lists.t_stride + i];
    const float* adj = s.adj + (int64_t)n * s.P * kAdjFloats;
    const float x[3] = {s.pts[r * 3 + 0], s.pts[r * 3 + 1], s.pts[r * 3 + 2]};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    gather_wave(s.lists, n, i, L, lane, s_raw, s_sorted, [&](int64_t q) { add_slot(adj, s.K, (int)q, x, acc); });
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = iso_wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) s.grad[r * 3 + c] = scale * acc[c];
    }
  }
}

inline int64_t adjoint_bytes(int64_t rows) { return iso_align16(4 * kAdjFloats * rows); }
inline int64_t flat_bytes(int64_t rows, int K) { return iso_align16(4 * rows * K); }

}  // namespace

// workspace of iso_pca_frames_backward: [G and m: R * 9 floats][the slots' targets: R * K int32][gather_lists.h's, with R
// target rows and R * K query rows], R = N * P
extern "C" int64_t iso_pca_frames_backward_work_bytes(int n_clouds, int64_t max_points, int K) {
  if (n_clouds < 0) n_clouds = 0;
  if (max_points < 0) max_points = 0;
  if (K < 1) K = 1;
  const int64_t R = (int64_t)n_clouds * max_points;
  return adjoint_bytes(R) + flat_bytes(R, K) + gather_workspace_bytes(R, R * K, max_points, n_clouds);
}

extern "C" int iso_pca_frames_backward(const float* points, const int64_t* lengths, const int64_t* idx, int n_clouds,
                                       int64_t max_points, int K, int disambiguate, const float* curvature,
                                       const float* frames, const float* grad_curvature, const float* grad_frames,
                                       void* work, int64_t work_bytes, float* grad_points_out, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && max_points >= 0 && K >= 1, ISO_ERR_INVALID, "iso_pca_frames_backward: bad sizes");
  ISO_REQUIRE((double)n_clouds * (double)max_points * (double)K < 2147483647.0, ISO_ERR_UNSUPPORTED,
              "iso_pca_frames_backward: 32-bit slot indices (n_clouds * max_points * K < 2^31 - 1)");
  if (n_clouds == 0 || max_points == 0) return ISO_OK;
  ISO_REQUIRE(points && idx && curvature && frames && grad_points_out, ISO_ERR_INVALID,
              "iso_pca_frames_backward: null pointer");
  ISO_REQUIRE(work && work_bytes >= iso_pca_frames_backward_work_bytes(n_clouds, max_points, K), ISO_ERR_WORKSPACE,
              "iso_pca_frames_backward: workspace too small");
  ISO_REQUIRE(((uintptr_t)work & 15) == 0, ISO_ERR_INVALID, "iso_pca_frames_backward: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = max_points, R = (int64_t)n_clouds * P;
  float* adj = (float*)work;
  int32_t* flat = (int32_t*)((char*)work + adjoint_bytes(R));
  const GatherWorkspace w = gather_carve((char*)work + adjoint_bytes(R) + flat_bytes(R, K), R, R * K);
  hipLaunchKernelGGL(k_pca_adjoint, dim3(iso_stream_grid(P, 256), n_clouds), dim3(256), 0, s, points, lengths, idx, P, K,
                     disambiguate ? 1 : 0, curvature, frames, grad_curvature, grad_frames, adj, flat);
  const GatherView lists{flat, w.cnt, w.off, w.slot, w.list, P * K, P, P * K, P};
  const int rc = gather_build(GatherViews{{lists, lists}}, 1, n_clouds, P * K, w, R, P, n_clouds, s);
  if (rc != ISO_OK) return rc;
  const PcaScatter a{points, lengths, adj, lists, w.heavy, w.heavy_count, grad_points_out, P, K};
  hipLaunchKernelGGL(k_pca_scatter, dim3(iso_capped_grid(P, 256, 4096), n_clouds), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_pca_scatter_heavy, dim3((int)(R < 2048 ? R : 2048)), dim3(64), 0, s, a);
  ISO_CHECK_LAUNCH("iso_pca_frames_backward");
  return ISO_OK;
}
