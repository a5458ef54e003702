// Point-to-triangle distances between packed point clouds and packed meshes on the cell grid of frnn.hip, written for
// gfx950.  Stands in for pytorch3d's point_face_distance / face_point_distance / point_mesh_face_distance as the
// reference calls them (include/isopoints.h section H for the call sites).
//
//   k_pf_prepare     : per face the centroid (padded per mesh: the grid's input), the radius R_t = the largest
//                      centroid-to-vertex distance, rounded up, and the mesh's R_max (integer atomicMax on the bits of a
//                      non-negative float: a max has no order)
//   k_pf_pack_tris   : the records of the point -> face walk: three float4 per face in the grid's sorted order,
//                      (v0, local face index as bits), (v1, -), (v2, -): a candidate is 48 contiguous bytes
//   k_pf_nearest<0>  : point -> face.  One lane per point walks the grid of the CENTROIDS with cell_grid.h's
//                      nearest_walk (the lane's own shells, then its whole wave); after shell rho every unseen face lies
//                      at least ring_reach(rho) - R_max away, so the walk stops once sqrt(best) <= ring_reach(rho) - R_max.
//   k_pf_nearest<1>  : face -> point.  The query walks the grid of the POINTS from the face's centroid; a point at distance
//                      d from the face is at most d + R_t from the centroid: stop once sqrt(best) + R_t <= ring_reach(rho).
//   k_pf_finish      : adds the workgroups' partial sums of a cloud in a fixed order
//   backward         : the query side is one term per query (k_pf_grad_query); the target side is a gather over the
//                      counting-sorted lists of gather_lists.h (integer atomics only), each list summed in ascending
//                      query order by its own lane (k_pf_grad_target) or by one wave (k_pf_grad_heavy).  No float
//                      atomics: two runs give the same bits.
//
// d2(p, t) is pf_closest() of pf_closest.h: a pure function of the pair (contraction off), so a result does not depend on the order of
// visits, the lane or the kernel that served the query.  Candidates are ordered by (d2, index).
#include <float.h>
#include "cell_grid.h"
#include "gather_lists.h"
#include "pf_closest.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPfBlock = 256;
constexpr int kPfMaxPartials = 1024;   // workgroups per cloud of k_pf_nearest = partial sums k_pf_finish adds
constexpr float kRadiusUp = 1.00001f;  // R_t is rounded up: the stop rules may only stop late
constexpr float kReachDown = 0.9999f;  // and the reach left after R is rounded down

__device__ __forceinline__ void load3(const float* __restrict__ src, float (&p)[3]) {
  p[0] = src[0]; p[1] = src[1]; p[2] = src[2];
}
__device__ __forceinline__ void load9(const float* __restrict__ src, float (&v)[9]) {
#pragma unroll
  for (int c = 0; c < 9; ++c) v[c] = src[c];
}

// ---- preparation ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pf_prepare(const float* __restrict__ tris, const int64_t* __restrict__ first,
                                                    const int64_t* __restrict__ len, int64_t n_tris, int64_t t_stride,
                                                    float* __restrict__ cen, float* __restrict__ rad,
                                                    float* __restrict__ rmax) {
  const int n = blockIdx.y;
  const int64_t f0 = first[n];
  const int64_t l = min(len[n], t_stride);
  float top = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = f0 + i;
    if (t < 0 || t >= n_tris) continue;
    float v[9];
    load9(tris + t * 9, v);
    float c[3], r2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ((v[k] + v[3 + k]) + v[6 + k]) / 3.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float dx = v[3 * k] - c[0], dy = v[3 * k + 1] - c[1], dz = v[3 * k + 2] - c[2];
      r2 = fmaxf(r2, (dx * dx + dy * dy) + dz * dz);
    }
    const float r = sqrtf(r2) * kRadiusUp;
#pragma unroll
    for (int k = 0; k < 3; ++k) cen[((int64_t)n * t_stride + i) * 3 + k] = c[k];
    rad[t] = r;
    if (r == r) top = fmaxf(top, r);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = fmaxf(top, __shfl_xor(top, o));
  // the bits of non-negative floats order as integers
  if ((threadIdx.x & 63) == 0 && top > 0.f) atomicMax(reinterpret_cast<int*>(rmax) + n, __float_as_int(top));
}

__global__ __launch_bounds__(256) void k_pf_pad_points(const float* __restrict__ points, const int64_t* __restrict__ first,
                                                       const int64_t* __restrict__ len, int64_t n_points,
                                                       int64_t p_stride, float* __restrict__ out) {
  const int n = blockIdx.y;
  const int64_t f0 = first[n];
  const int64_t l = min(len[n], p_stride);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = f0 + i;
    if (q < 0 || q >= n_points) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[((int64_t)n * p_stride + i) * 3 + k] = points[q * 3 + k];
  }
}

__global__ __launch_bounds__(256) void k_pf_pack_tris(const float* __restrict__ tris, const int64_t* __restrict__ first,
                                                      const int64_t* __restrict__ len, const int32_t* __restrict__ sorted_idx,
                                                      int64_t n_tris, int64_t t_stride, float4* __restrict__ rec) {
  const int n = blockIdx.y;
  const int64_t f0 = first[n];
  const int64_t l = min(len[n], t_stride);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < l; i += (int64_t)gridDim.x * blockDim.x) {
    const int li = sorted_idx[(int64_t)n * t_stride + i];
    const int64_t t = f0 + li;
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (li >= 0 && li < l && t >= 0 && t < n_tris) load9(tris + t * 9, v);
    float4* o = rec + ((int64_t)n * t_stride + i) * 3;
    o[0] = make_float4(v[0], v[1], v[2], __int_as_float(li));
    o[1] = make_float4(v[3], v[4], v[5], 0.f);
    o[2] = make_float4(v[6], v[7], v[8], 0.f);
  }
}

// ---- the search -------------------------------------------------------------------------------------------------
struct PfSearch {
  const float* points;        // (P,3) packed
  const int64_t* pts_first;   // (N)
  const int64_t* pts_len;
  const float* tris;          // (T,9) packed
  const int64_t* tris_first;
  const int64_t* tris_len;
  const float4* rec;          // DIR 0: (N,t_stride,3) face records; DIR 1: (N,p_stride) point records
  const int32_t* off;         // the target grid's cell offsets (N,g_stride)
  const float* params;
  const float* cen;           // (N,t_stride,3)
  const float* rad;           // (T)
  const float* rmax;          // (N)
  float* d2_out;              // (Q)
  int32_t* idx_out;           // (Q) packed index of the target, -1 without one
  float* partials;            // (N, gridDim.x)
  int64_t n_points, n_tris, t_stride, target_stride, g_stride;
  float min_area;
};

// what the walk knows of a query: where it stands (p: the point, or the face's centroid), its face (DIR 1) and the
// radius R that the stop rule takes off the reach (DIR 0: the mesh's R_max; DIR 1: the face's R_t)
struct PfQuery { float p[3]; float v[9]; float R; };

template <int DIR>
__device__ __forceinline__ void pf_load_query(const PfSearch& a, int n, int64_t i, int64_t q, PfQuery& qu) {
  if (DIR == 0) {
    load3(a.points + q * 3, qu.p);
    qu.R = a.rmax[n];
  } else {
    load9(a.tris + q * 9, qu.v);
    load3(a.cen + ((int64_t)n * a.t_stride + i) * 3, qu.p);
    qu.R = a.rad[q];
  }
}

// the records [i0, i1) of cloud n against the query; (d2, local index) order
template <int DIR>
__device__ __forceinline__ void pf_scan(const float4* __restrict__ rec, int64_t i0, int64_t i1, const PfQuery& qu,
                                        float min_area, float& bd, int& bi) {
  for (int64_t i = i0; i < i1; ++i) {
    float d2, bw[3];
    int oi;
    if (DIR == 0) {
      const float4 r0 = rec[i * 3], r1 = rec[i * 3 + 1], r2 = rec[i * 3 + 2];
      const float v[9] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z};
      d2 = pf_closest(qu.p, v, min_area, bw);
      oi = __float_as_int(r0.w);
    } else {
      const float4 r = rec[i];
      const float p[3] = {r.x, r.y, r.z};
      d2 = pf_closest(p, qu.v, min_area, bw);
      oi = __float_as_int(r.w);
    }
    if (pair_lt(d2, oi, bd, bi)) { bd = d2; bi = oi; }
  }
}

// every target not seen after shell rho is farther than the best: the reach less R, rounded down, covers sqrt(best)
__device__ __forceinline__ bool pf_closed(float bd, int rho, float cell, float R) {
  const float m = (ring_reach(rho, cell) - R) * kReachDown;
  return bd < FLT_MAX && m > 0.f && bd <= m * m;
}

template <int DIR>
__global__ __launch_bounds__(kPfBlock) void k_pf_nearest(PfSearch a) {
  __shared__ float s_sum[kPfBlock / 64];
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int64_t n_q = DIR == 0 ? a.n_points : a.n_tris;
  const int64_t q_first = DIR == 0 ? a.pts_first[n] : a.tris_first[n];
  const int64_t q_len = DIR == 0 ? a.pts_len[n] : min(a.tris_len[n], a.t_stride);
  const int64_t t_first = DIR == 0 ? a.tris_first[n] : a.pts_first[n];
  const int64_t len2 = min(DIR == 0 ? a.tris_len[n] : a.pts_len[n], a.target_stride);
  const float4* rec = a.rec + (int64_t)n * a.target_stride * (DIR == 0 ? 3 : 1);
  const Grid3 g = grid3_load(a.params, n);
  const int32_t* offn = a.off + (int64_t)n * a.g_stride;
  float acc = 0.f;

  // the loop bound is the same in every lane of a wave: the lanes of a wave finish its open queries together
  for (int64_t t0 = (int64_t)blockIdx.x * kPfBlock; t0 < q_len; t0 += (int64_t)gridDim.x * kPfBlock) {
    const int64_t t = t0 + threadIdx.x;
    const int64_t q = q_first + t;
    const bool row = t < q_len && q >= 0 && q < n_q;
    PfQuery qu;
    qu.p[0] = qu.p[1] = qu.p[2] = 0.f;
    qu.R = 0.f;
    if (row && len2 > 0) pf_load_query<DIR>(a, n, t, q, qu);
    const bool live = row && len2 > 0 && qu.p[0] == qu.p[0] && qu.p[1] == qu.p[1] && qu.p[2] == qu.p[2];
    float bd = FLT_MAX;
    int bi = 0x7fffffff;
    nearest_walk(
        g, offn, len2, lane, live, qu, qu.p[0], qu.p[1], qu.p[2],
        [&](const PfQuery& w, int64_t i0, int64_t i1, float& d, int& i) { pf_scan<DIR>(rec, i0, i1, w, a.min_area, d, i); },
        [&](const PfQuery& w, float d, int rho) { return pf_closed(d, rho, g.cell, w.R); },
        [&](int src, PfQuery& wq) {   // the wave reloads the open query: cheaper than shuffling up to 13 floats
          const int64_t wt = t0 + (threadIdx.x - lane) + src;
          pf_load_query<DIR>(a, n, wt, q_first + wt, wq);
        },
        bd, bi);
    if (row) {
      const bool found = bd < FLT_MAX;
      const float d2 = found ? bd : 0.f;
      a.d2_out[q] = d2;
      a.idx_out[q] = found ? (int32_t)(t_first + bi) : -1;
      acc += d2;
    }
  }
  acc = iso_wave_sum(acc);
  if (lane == 0) s_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = s_sum[0];
#pragma unroll
    for (int w = 1; w < kPfBlock / 64; ++w) s += s_sum[w];
    a.partials[(int64_t)n * gridDim.x + blockIdx.x] = s;
  }
}

// sums_out[n]: the partials of cloud n in 64 contiguous chunks, each added in index order by one lane, then the 64 chunk
// sums by one butterfly
__global__ __launch_bounds__(64) void k_pf_finish(const float* __restrict__ partials, int n_part,
                                                  float* __restrict__ sums_out) {
  const int n = blockIdx.x, l = threadIdx.x;
  const int chunk = (n_part + 63) / 64;
  float s = 0.f;
  for (int k = 0; k < chunk; ++k) {
    const int i = l * chunk + k;
    if (i < n_part) s += partials[(int64_t)n * n_part + i];
  }
  s = iso_wave_sum(s);
  if (l == 0) sums_out[n] = s;
}

// ---- backward ---------------------------------------------------------------------------------------------------
// Query q chose target idx[q] (packed indices, so one flat list serves the whole batch).  DIR 0: queries are points,
// targets faces; DIR 1: queries are faces, targets points.  With r = p - c and b the weights of the closest point c:
// d d2 / d p = 2 r, d d2 / d v_k = -2 b_k r, each times the query's weight w[q].
struct PfBack {
  const float* points;
  const float* tris;
  const float* w;       // (Q)
  float* grad_query;    // DIR 0: (P,3); DIR 1: (T,9); null = not wanted
  float* grad_target;   // DIR 0: (T,9); DIR 1: (P,3); null = not wanted
  int64_t n_q, n_t;
  GatherView lists;     // one cloud: idx (Q) = the packed target of each query
  int32_t* heavy;       // (n_t)
  int32_t* heavy_count;
  float min_area;
};

// r = p - c of the pair and the weights of c
template <int DIR>
__device__ __forceinline__ void pf_pair(const PfBack& a, int64_t q, int64_t i, float (&r)[3], float (&bw)[3]) {
  float p[3], v[9];
  load3(a.points + (DIR == 0 ? q : i) * 3, p);
  load9(a.tris + (DIR == 0 ? i : q) * 9, v);
  pf_closest(p, v, a.min_area, bw);
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = p[k] - ((bw[0] * v[k] + bw[1] * v[3 + k]) + bw[2] * v[6 + k]);
}

// what query q adds to its target i: DIR 0 nine floats of the face, DIR 1 three of the point
template <int DIR>
__device__ __forceinline__ void pf_add_target(const PfBack& a, int64_t q, int64_t i, float (&acc)[DIR == 0 ? 9 : 3]) {
  float r[3], bw[3];
  pf_pair<DIR>(a, q, i, r, bw);
  const float w2 = 2.0f * a.w[q];
  if (DIR == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float s = -(w2 * bw[k]);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * k + c] += s * r[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += w2 * r[c];
  }
}

template <int DIR>
__global__ __launch_bounds__(256) void k_pf_grad_query(PfBack a) {
  constexpr int W = DIR == 0 ? 3 : 9;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.n_q; q += (int64_t)gridDim.x * blockDim.x) {
    float out[W];
#pragma unroll
    for (int c = 0; c < W; ++c) out[c] = 0.f;
    const int i = a.lists.idx[q];
    if (i >= 0 && i < a.n_t) {
      float r[3], bw[3];
      pf_pair<DIR>(a, q, i, r, bw);
      const float w2 = 2.0f * a.w[q];
      if (DIR == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = w2 * r[c];
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float s = -(w2 * bw[k]);
#pragma unroll
          for (int c = 0; c < 3; ++c) out[3 * k + c] = s * r[c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < W; ++c) a.grad_query[q * W + c] = out[c];
  }
}

// One lane per target: a list of up to kLightList queries is summed here in ascending query order, a longer one is
// left to k_pf_grad_heavy (this kernel writes zero, that one adds the list's sum).
template <int DIR>
__global__ __launch_bounds__(256) void k_pf_grad_target(PfBack a) {
  constexpr int W = DIR == 0 ? 9 : 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_t; i += (int64_t)gridDim.x * blockDim.x) {
    float acc[W];
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = 0.f;
    const int L = a.lists.cnt[i];
    if (L > kLightList) {
      a.heavy[atomicAdd(a.heavy_count, 1)] = (int32_t)i;   // the order of this list decides nothing: one wave per entry
    } else if (L > 0) {
      gather_lane(gather_list(a.lists, 0, i), L, [&](int q) { pf_add_target<DIR>(a, q, i, acc); });
    }
#pragma unroll
    for (int c = 0; c < W; ++c) a.grad_target[i * W + c] = acc[c];
  }
}

// One wave per long list (gather_wave): every lane's sum runs in ascending query order and the 64 sums are added by the
// same butterfly, a fixed order.
template <int DIR>
__global__ __launch_bounds__(64) void k_pf_grad_heavy(PfBack a) {
  constexpr int W = DIR == 0 ? 9 : 3;
  __shared__ int32_t s_raw[kSortList], s_sorted[kSortList];
  const int lane = threadIdx.x;
  const int count = *a.heavy_count;
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int i = a.heavy[w];
    const int L = a.lists.cnt[i];
    float acc[W];
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = 0.f;
    gather_wave(a.lists, 0, i, L, lane, s_raw, s_sorted, [&](int64_t q) { pf_add_target<DIR>(a, q, i, acc); });
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = iso_wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < W; ++c) a.grad_target[(int64_t)i * W + c] += acc[c];
    }
  }
}

template <int DIR>
void pf_launch_backward(const PfBack& a, bool query_side, bool target_side, int gq, int gt, int gh, hipStream_t s) {
  if (query_side) hipLaunchKernelGGL(k_pf_grad_query<DIR>, dim3(gq), dim3(256), 0, s, a);
  if (target_side) {
    hipLaunchKernelGGL(k_pf_grad_target<DIR>, dim3(gt), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_pf_grad_heavy<DIR>, dim3(gh), dim3(64), 0, s, a);
  }
}

}  // namespace

extern "C" int iso_pfdist_prepare(const float* points, const int64_t* pts_first, const int64_t* pts_len,
                                  const float* tris, const int64_t* tris_first, const int64_t* tris_len, int n_clouds,
                                  int64_t n_points, int64_t n_tris, int64_t p_stride, int64_t t_stride,
                                  float* points_padded_out, float* centroids_out, float* radius_out, float* rmax_out,
                                  void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && n_points >= 0 && n_tris >= 0 && p_stride >= 0 && t_stride >= 0, ISO_ERR_INVALID,
              "iso_pfdist_prepare: bad sizes");
  if (n_clouds == 0) return ISO_OK;
  hipStream_t s = (hipStream_t)stream;
  if (points_padded_out && p_stride > 0 && n_points > 0) {
    ISO_REQUIRE(points && pts_first && pts_len, ISO_ERR_INVALID, "iso_pfdist_prepare: null pointer");
    hipLaunchKernelGGL(k_pf_pad_points, dim3(iso_capped_grid(p_stride, kPfBlock, 4096), n_clouds), dim3(256), 0, s, points, pts_first,
                       pts_len, n_points, p_stride, points_padded_out);
  }
  if (centroids_out) {
    ISO_REQUIRE(tris_first && tris_len && radius_out && rmax_out && (tris || n_tris == 0), ISO_ERR_INVALID,
                "iso_pfdist_prepare: null pointer");
    iso_zero_words(rmax_out, n_clouds, s);
    if (t_stride > 0 && n_tris > 0)
      hipLaunchKernelGGL(k_pf_prepare, dim3(iso_capped_grid(t_stride, kPfBlock, 4096), n_clouds), dim3(256), 0, s, tris, tris_first,
                         tris_len, n_tris, t_stride, centroids_out, radius_out, rmax_out);
  }
  ISO_CHECK_LAUNCH("iso_pfdist_prepare");
  return ISO_OK;
}

// workspace of iso_pfdist_forward: [records: N * target_stride float4, three per face][partials: N * grid floats]
extern "C" int64_t iso_pfdist_forward_workspace_bytes(int direction, int n_clouds, int64_t q_stride,
                                                      int64_t target_stride) {
  if (n_clouds < 0) n_clouds = 0;
  if (q_stride < 0) q_stride = 0;
  if (target_stride < 0) target_stride = 0;
  return (direction == 0 ? 48 : 16) * (int64_t)n_clouds * target_stride +
         iso_align16((int64_t)n_clouds * iso_capped_grid(q_stride, kPfBlock, kPfMaxPartials) * 4) + 16;
}

extern "C" int iso_pfdist_forward(int direction, const float* points, const int64_t* pts_first, const int64_t* pts_len,
                                  const float* tris, const int64_t* tris_first, const int64_t* tris_len,
                                  const float* sorted_targets, const int32_t* sorted_idx, const int32_t* off,
                                  const float* grid_params, const float* centroids, const float* radius,
                                  const float* rmax, float min_triangle_area, float* d2_out, int32_t* idx_out,
                                  float* sums_out, int n_clouds, int64_t n_points, int64_t n_tris, int64_t p_stride,
                                  int64_t t_stride, int64_t g_stride, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  ISO_REQUIRE(direction == 0 || direction == 1, ISO_ERR_INVALID, "iso_pfdist_forward: direction is 0 or 1");
  ISO_REQUIRE(n_clouds >= 0 && n_points >= 0 && n_tris >= 0 && p_stride >= 0 && t_stride >= 0 && g_stride >= 0,
              ISO_ERR_INVALID, "iso_pfdist_forward: bad sizes");
  ISO_REQUIRE(n_points < 0x7fffffff && n_tris < 0x7fffffff, ISO_ERR_UNSUPPORTED, "iso_pfdist_forward: 32-bit indices");
  ISO_REQUIRE(min_triangle_area >= 0.f, ISO_ERR_INVALID, "iso_pfdist_forward: min_triangle_area is negative");
  if (n_clouds == 0) return ISO_OK;
  const int64_t q_stride = direction == 0 ? p_stride : t_stride;
  const int64_t target_stride = direction == 0 ? t_stride : p_stride;
  const int64_t n_q = direction == 0 ? n_points : n_tris;
  ISO_REQUIRE(sums_out && pts_first && pts_len && tris_first && tris_len, ISO_ERR_INVALID,
              "iso_pfdist_forward: null pointer");
  ISO_REQUIRE((d2_out && idx_out) || n_q == 0, ISO_ERR_INVALID, "iso_pfdist_forward: null pointer");
  ISO_REQUIRE(points || n_points == 0, ISO_ERR_INVALID, "iso_pfdist_forward: null pointer");
  ISO_REQUIRE((tris && centroids && radius) || n_tris == 0, ISO_ERR_INVALID, "iso_pfdist_forward: null pointer");
  ISO_REQUIRE((sorted_targets && sorted_idx) || target_stride == 0, ISO_ERR_INVALID, "iso_pfdist_forward: null pointer");
  ISO_REQUIRE(off && grid_params && rmax, ISO_ERR_INVALID, "iso_pfdist_forward: null pointer");
  ISO_REQUIRE(workspace && workspace_bytes >= iso_pfdist_forward_workspace_bytes(direction, n_clouds, q_stride, target_stride),
              ISO_ERR_WORKSPACE, "iso_pfdist_forward: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "iso_pfdist_forward: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  float4* rec = reinterpret_cast<float4*>(workspace);
  float* partials = reinterpret_cast<float*>((char*)workspace + (direction == 0 ? 48 : 16) * (int64_t)n_clouds * target_stride);
  const int gx = iso_capped_grid(q_stride, kPfBlock, kPfMaxPartials);
  PfSearch a{points, pts_first, pts_len, tris, tris_first, tris_len, rec, off, grid_params, centroids, radius, rmax,
             d2_out, idx_out, partials, n_points, n_tris, t_stride, target_stride, g_stride, min_triangle_area};
  if (direction == 0) {
    if (t_stride > 0)
      hipLaunchKernelGGL(k_pf_pack_tris, dim3(iso_capped_grid(t_stride, kPfBlock, 4096), n_clouds), dim3(256), 0, s, tris, tris_first,
                         tris_len, sorted_idx, n_tris, t_stride, rec);
    hipLaunchKernelGGL(k_pf_nearest<0>, dim3(gx, n_clouds), dim3(kPfBlock), 0, s, a);
  } else {
    pack_xyzi(sorted_targets, sorted_idx, pts_len, n_clouds, p_stride, rec, s);
    hipLaunchKernelGGL(k_pf_nearest<1>, dim3(gx, n_clouds), dim3(kPfBlock), 0, s, a);
  }
  hipLaunchKernelGGL(k_pf_finish, dim3(n_clouds), dim3(64), 0, s, partials, gx, sums_out);
  ISO_CHECK_LAUNCH("iso_pfdist_forward");
  return ISO_OK;
}

// workspace of iso_pfdist_backward: gather_lists.h's, with n_t target rows and n_q query rows
extern "C" int64_t iso_pfdist_backward_workspace_bytes(int direction, int64_t n_points, int64_t n_tris) {
  if (n_points < 0) n_points = 0;
  if (n_tris < 0) n_tris = 0;
  const int64_t n_q = direction == 0 ? n_points : n_tris, n_t = direction == 0 ? n_tris : n_points;
  return gather_workspace_bytes(n_t, n_q, n_t, 1);
}

extern "C" int iso_pfdist_backward(int direction, const float* points, const float* tris, const int32_t* idx,
                                   const float* weights, float min_triangle_area, float* grad_points, float* grad_tris,
                                   int64_t n_points, int64_t n_tris, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  ISO_REQUIRE(direction == 0 || direction == 1, ISO_ERR_INVALID, "iso_pfdist_backward: direction is 0 or 1");
  ISO_REQUIRE(n_points >= 0 && n_tris >= 0, ISO_ERR_INVALID, "iso_pfdist_backward: bad sizes");
  ISO_REQUIRE(n_points < 0x7fffffff && n_tris < 0x7fffffff, ISO_ERR_UNSUPPORTED, "iso_pfdist_backward: 32-bit indices");
  const int64_t n_q = direction == 0 ? n_points : n_tris, n_t = direction == 0 ? n_tris : n_points;
  float* grad_query = direction == 0 ? grad_points : grad_tris;
  float* grad_target = direction == 0 ? grad_tris : grad_points;
  const bool query_side = grad_query && n_q > 0, target_side = grad_target && n_t > 0;
  if (!query_side && !target_side) return ISO_OK;
  ISO_REQUIRE(n_q == 0 || (idx && weights), ISO_ERR_INVALID, "iso_pfdist_backward: null pointer");
  ISO_REQUIRE((points || n_points == 0) && (tris || n_tris == 0), ISO_ERR_INVALID, "iso_pfdist_backward: null pointer");
  ISO_REQUIRE(workspace && workspace_bytes >= iso_pfdist_backward_workspace_bytes(direction, n_points, n_tris),
              ISO_ERR_WORKSPACE, "iso_pfdist_backward: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "iso_pfdist_backward: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  const GatherWorkspace w = gather_carve(workspace, n_t, n_q);
  const GatherView lists{idx, w.cnt, w.off, w.slot, w.list, n_q, n_t, n_q, n_t};
  PfBack a{points, tris, weights, grad_query, grad_target, n_q, n_t, lists, w.heavy, w.heavy_count, min_triangle_area};
  const int gq = iso_capped_grid(n_q, kPfBlock, 4096), gt = iso_capped_grid(n_t, kPfBlock, 4096);
  const int gh = (int)(n_t < 2048 ? (n_t < 1 ? 1 : n_t) : 2048);
  if (target_side) {
    const int rc = gather_build(GatherViews{{lists, lists}}, 1, 1, n_q, w, n_t, n_t, 1, s);
    if (rc != ISO_OK) return rc;
  }
  if (direction == 0) pf_launch_backward<0>(a, query_side, target_side, gq, gt, gh, s);
  else pf_launch_backward<1>(a, query_side, target_side, gq, gt, gh, s);
  ISO_CHECK_LAUNCH("iso_pfdist_backward");
  return ISO_OK;
}
