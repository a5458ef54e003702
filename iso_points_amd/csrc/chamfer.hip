// Chamfer distance between two point clouds on the cell grid of frnn.hip, written for gfx950.
// Stands in for pytorch3d.loss.chamfer_distance as the reference calls it (include/isopoints.h
// section G for the call sites).
//
//   k_cham_nearest  : one lane per query runs cell_grid.h's nearest_walk (the walk, the d2 expression and the
//                     (d2, index) order k_query uses, with K = 1 and no radius; a query still open after
//                     kRingCap further shells is finished by its whole WAVE in the same launch).  The lane
//                     then forms the normal term and the workgroup reduces both sums in a fixed order.
//   k_cham_finish   : adds the workgroups' partial sums of a cloud in a fixed order (64 chunks in index order)
//   backward        : gather_lists.h sorts the other cloud's nearest indices by target (integer atomics only);
//                     k_cham_grad sums each target's list in ascending query order, k_cham_grad_heavy serves the
//                     long lists with one wave each.  Both clouds' gradients run in the same launches
//                     (blockIdx.z = the side).  No float atomics: two runs give the same bits.
#include <float.h>
#include "cell_grid.h"
#include "gather_lists.h"

#pragma clang fp contract(off)

namespace {

constexpr int kNearBlock = 256;
constexpr int kMaxPartials = 4096;   // workgroups per cloud of k_cham_nearest = partial sums k_cham_finish adds
constexpr float kNormEps = 1e-6f;    // torch.nn.functional.cosine_similarity's eps

// 1 - |cos(a, b)|, cos = a.b / (max(|a|, eps) max(|b|, eps))
__device__ __forceinline__ float normal_term(const float* __restrict__ a, const float* __restrict__ b) {
  const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
  const float la = sqrtf((ax * ax + ay * ay) + az * az), lb = sqrtf((bx * bx + by * by) + bz * bz);
  const float dot = (ax * bx + ay * by) + az * bz;
  return 1.0f - fabsf(dot / (fmaxf(la, kNormEps) * fmaxf(lb, kNormEps)));
}

struct Pt { float x, y, z; };

template <bool NORMALS>
__global__ __launch_bounds__(kNearBlock) void k_cham_nearest(
    const float* __restrict__ x, const int64_t* __restrict__ x_len, const float4* __restrict__ xyzi,
    const int64_t* __restrict__ y_len, const int32_t* __restrict__ off, const float* __restrict__ params,
    const float* __restrict__ x_normals, const float* __restrict__ y_normals, float* __restrict__ d2_out,
    int32_t* __restrict__ idx_out, float* __restrict__ nterm_out, float* __restrict__ partials, int64_t p1,
    int64_t p2, int64_t g_stride) {
  __shared__ float s_sum[kNearBlock / 64][2];
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const float4* s4 = xyzi + (int64_t)n * p2;
  const int64_t len2 = y_len ? y_len[n] : p2;
  const int64_t len1 = x_len ? x_len[n] : p1;
  const Grid3 g = grid3_load(params, n);
  const int32_t* offn = off + (int64_t)n * g_stride;
  float acc_d = 0.f, acc_n = 0.f;

  // the loop bound is the same in every lane of a wave: the lanes of a wave finish its open queries together
  for (int64_t t0 = (int64_t)blockIdx.x * kNearBlock; t0 < p1; t0 += (int64_t)gridDim.x * kNearBlock) {
    const int64_t t = t0 + threadIdx.x;
    const bool row = t < p1;
    Pt q = {0.f, 0.f, 0.f};
    if (row && t < len1 && len2 > 0) {
      const float* qp = x + ((int64_t)n * p1 + t) * 3;
      q.x = qp[0]; q.y = qp[1]; q.z = qp[2];
    }
    const bool live = row && t < len1 && len2 > 0 && q.x == q.x && q.y == q.y && q.z == q.z;
    float bd = FLT_MAX;
    int bi = 0x7fffffff;
    nearest_walk(
        g, offn, len2, lane, live, q, q.x, q.y, q.z,
        [&](const Pt& w, int64_t i0, int64_t i1, float& d, int& i) {
          scan_run2(s4, i0, i1, w.x, w.y, w.z, [&](float d2, int oi) {
            if (pair_lt(d2, oi, d, i)) { d = d2; i = oi; }
          });
        },
        [&](const Pt&, float d, int rho) {
          const float reach = ring_reach(rho, g.cell);
          return d < FLT_MAX && d <= reach * reach;
        },
        [&](int src, Pt& w) { w.x = __shfl(q.x, src); w.y = __shfl(q.y, src); w.z = __shfl(q.z, src); }, bd, bi);
    if (row) {
      const bool found = bd < FLT_MAX;
      const float d2 = found ? bd : 0.f;
      float nt = 0.f;
      if (NORMALS && found)
        nt = normal_term(x_normals + ((int64_t)n * p1 + t) * 3, y_normals + ((int64_t)n * p2 + bi) * 3);
      if (d2_out) d2_out[(int64_t)n * p1 + t] = d2;
      idx_out[(int64_t)n * p1 + t] = found ? bi : -1;
      if (NORMALS && nterm_out) nterm_out[(int64_t)n * p1 + t] = nt;
      acc_d += d2;
      acc_n += nt;
    }
  }
  acc_d = iso_wave_sum(acc_d);
  acc_n = iso_wave_sum(acc_n);
  if (lane == 0) { s_sum[threadIdx.x >> 6][0] = acc_d; s_sum[threadIdx.x >> 6][1] = acc_n; }
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = s_sum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kNearBlock / 64; ++w) s += s_sum[w][threadIdx.x];
    partials[((int64_t)n * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = s;
  }
}

// sums_out[n] = {sum d2, sum normal term}: the partials of cloud n in 64 contiguous chunks, each added in index order by
// one lane, then the 64 chunk sums added in order
__global__ __launch_bounds__(128) void k_cham_finish(const float* __restrict__ partials, int n_part,
                                                     float* __restrict__ sums_out) {
  __shared__ float s_p[kMaxPartials * 2];
  __shared__ float s_c[2][64];
  const int n = blockIdx.x;
  for (int i = threadIdx.x; i < n_part * 2; i += 128) s_p[i] = partials[(int64_t)n * n_part * 2 + i];
  __syncthreads();
  const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int chunk = (n_part + 63) / 64;
  float s = 0.f;
  for (int k = 0; k < chunk; ++k) {
    const int i = l * chunk + k;
    if (i < n_part) s += s_p[i * 2 + q];
  }
  s_c[q][l] = s;
  __syncthreads();
  if (l == 0) {
    float t = 0.f;
    for (int k = 0; k < 64; ++k) t += s_c[q][k];
    sums_out[n * 2 + q] = t;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
// One side of the backward pass: cloud A (p1 rows, the gradient's owner) and cloud B (p2 rows).  idx_b[j] = the row of A
// that row j of B chose: B's rows are the queries of the gather `lists`, A's rows its targets.  Both sides (x as A, y as
// A) run in the same launches, blockIdx.z picks the side.  Count and offset rows have the common stride pm = max(P1, P2),
// so that one batched prefix sum serves both sides.
struct Side {
  const float* a;        // (N,p1,3)
  const float* b;        // (N,p2,3)
  const float* an;       // normals of A or null
  const float* bn;
  const int64_t* a_len;
  const int32_t* idx_a;  // (N,p1): row of B chosen by row i of A
  const float* g_own;    // (N) scale of A's own terms
  const float* g_other;  // (N) scale of the terms of B's rows
  const float* gn_own;
  const float* gn_other;
  float* grad_a;
  float* grad_an;        // null: the normals' gradient is not wanted
  int64_t p1, p2;
  GatherView lists;      // idx = idx_b (N,p2), rows of stride p2 (queries) and pm (targets)
  int32_t* heavy;        // (N*p1)
  int32_t* heavy_count;
};
struct Sides { Side d[2]; };

// d(1 - |cos(a, b)|) / da
__device__ __forceinline__ void normal_term_grad(const float (&a)[3], const float* __restrict__ b, float (&out)[3]) {
  const float bx = b[0], by = b[1], bz = b[2];
  const float la = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), lb = sqrtf((bx * bx + by * by) + bz * bz);
  const float ca = fmaxf(la, kNormEps), cb = fmaxf(lb, kNormEps);
  const float c = ((a[0] * bx + a[1] * by) + a[2] * bz) / (ca * cb);
  const float sgn = c > 0.f ? -1.f : (c < 0.f ? 1.f : 0.f);       // -sign(cos)
  const float k1 = sgn / (ca * cb);
  const float k2 = (la >= kNormEps) ? sgn * c / (la * ca) : 0.f;  // the clamped norm is a constant
  out[0] = k1 * bx - k2 * a[0];
  out[1] = k1 * by - k2 * a[1];
  out[2] = k1 * bz - k2 * a[2];
}

// what row j of B adds to row i of A: (a_i - b_j) to pos, d(1 - |cos(an_i, bn_j)|)/d an_i to nrm
template <bool NORMALS>
__device__ __forceinline__ void add_pair(const Side& s, int n, const float (&ai)[3], const float (&ani)[3], int64_t j,
                                         float (&pos)[3], float (&nrm)[3]) {
  const float* bj = s.b + ((int64_t)n * s.p2 + j) * 3;
  pos[0] += ai[0] - bj[0]; pos[1] += ai[1] - bj[1]; pos[2] += ai[2] - bj[2];
  if (NORMALS) {
    float gn[3];
    normal_term_grad(ani, s.bn + ((int64_t)n * s.p2 + j) * 3, gn);
    nrm[0] += gn[0]; nrm[1] += gn[1]; nrm[2] += gn[2];
  }
}

// grad_a[i] = 2 g_own (a_i - b[idx_a[i]]) + 2 g_other sum_{j: idx_b[j] = i} (a_i - b_j), and the same two parts for the
// normals.  One lane per row of A; a list longer than kLightList is left to k_cham_grad_heavy (this kernel writes the row's
// own part, that one adds the list's).
template <bool NORMALS>
__global__ __launch_bounds__(256) void k_cham_grad(Sides both) {
  const Side s = blockIdx.z ? both.d[1] : both.d[0];
  const int n = blockIdx.y;
  const int64_t len = s.a_len ? s.a_len[n] : s.p1;
  const float go = 2.0f * s.g_own[n], gt = 2.0f * s.g_other[n];
  const float no = NORMALS ? s.gn_own[n] : 0.f, nt = NORMALS ? s.gn_other[n] : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.p1; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = (int64_t)n * s.p1 + i;
    const int64_t c_row = (int64_t)n * s.lists.t_stride + i;
    float gp[3] = {0.f, 0.f, 0.f}, gq[3] = {0.f, 0.f, 0.f};
    if (i < len) {
      float ai[3], ani[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) ai[c] = s.a[r * 3 + c];
      if (NORMALS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ani[c] = s.an[r * 3 + c];
      }
      const int own = s.idx_a[r];
      if (own >= 0) {
        float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
        add_pair<NORMALS>(s, n, ai, ani, own, pos, nrm);
#pragma unroll
        for (int c = 0; c < 3; ++c) { gp[c] = go * pos[c]; gq[c] = no * nrm[c]; }
      }
      const int L = s.lists.cnt[c_row];
      if (L > kLightList) {
        s.heavy[atomicAdd(s.heavy_count, 1)] = (int32_t)r;  // the order of this list decides nothing: one wave per entry
      } else if (L > 0) {
        float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
        gather_lane(gather_list(s.lists, n, i), L, [&](int j) { add_pair<NORMALS>(s, n, ai, ani, j, pos, nrm); });
#pragma unroll
        for (int c = 0; c < 3; ++c) { gp[c] += gt * pos[c]; gq[c] += nt * nrm[c]; }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s.grad_a[r * 3 + c] = gp[c];
    if (NORMALS && s.grad_an) {
#pragma unroll
      for (int c = 0; c < 3; ++c) s.grad_an[r * 3 + c] = gq[c];
    }
  }
}

// One wave per long list (gather_wave): every lane's sum runs in ascending query order and the 64 sums are added by the
// same butterfly, a fixed order.
template <bool NORMALS>
__global__ __launch_bounds__(64) void k_cham_grad_heavy(Sides both) {
  __shared__ int32_t s_raw[kSortList], s_sorted[kSortList];
  const Side s = blockIdx.z ? both.d[1] : both.d[0];
  const int lane = threadIdx.x;
  const int count = *s.heavy_count;
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int64_t r = s.heavy[w];
    const int n = (int)(r / s.p1);
    const int i = (int)(r - (int64_t)n * s.p1);
    const int L = s.lists.cnt[(int64_t)n * s.lists.t_stride + i];
    float ai[3], ani[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) ai[c] = s.a[r * 3 + c];
    if (NORMALS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ani[c] = s.an[r * 3 + c];
    }
    float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
    gather_wave(s.lists, n, i, L, lane, s_raw, s_sorted,
                [&](int64_t j) { add_pair<NORMALS>(s, n, ai, ani, j, pos, nrm); });
#pragma unroll
    for (int c = 0; c < 3; ++c) { pos[c] = iso_wave_sum(pos[c]); nrm[c] = iso_wave_sum(nrm[c]); }
    if (lane == 0) {
      const float gt = 2.0f * s.g_other[n];
#pragma unroll
      for (int c = 0; c < 3; ++c) s.grad_a[r * 3 + c] += gt * pos[c];
      if (NORMALS && s.grad_an) {
        const float nt = s.gn_other[n];
#pragma unroll
        for (int c = 0; c < 3; ++c) s.grad_an[r * 3 + c] += nt * nrm[c];
      }
    }
  }
}

}  // namespace

// workspace of iso_chamfer_nearest: [candidate records: N*P2 float4][partials: N * grid * 2 floats]
extern "C" int64_t iso_chamfer_nearest_workspace_bytes(int n_clouds, int64_t p1, int64_t p2) {
  if (n_clouds < 0) n_clouds = 0;
  if (p1 < 0) p1 = 0;
  if (p2 < 0) p2 = 0;
  return 16 * (int64_t)n_clouds * p2 + iso_align16((int64_t)n_clouds * iso_capped_grid(p1, kNearBlock, kMaxPartials) * 2 * 4) + 16;
}

extern "C" int iso_chamfer_nearest(const float* x, const int64_t* x_lengths, const float* sorted_y,
                                   const int32_t* sorted_idx_y, const int64_t* y_lengths, const int32_t* off,
                                   const float* grid_params, const float* x_normals, const float* y_normals,
                                   float* d2_out, int32_t* idx_out, float* nterm_out, float* sums_out, int n_clouds,
                                   int64_t p1, int64_t p2, int64_t g_stride, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && p1 >= 0 && p2 >= 0 && g_stride >= 0, ISO_ERR_INVALID, "iso_chamfer_nearest: bad sizes");
  ISO_REQUIRE(p1 < 0x7fffffff && p2 < 0x7fffffff, ISO_ERR_UNSUPPORTED, "iso_chamfer_nearest: 32-bit point indices");
  if (n_clouds == 0) return ISO_OK;
  ISO_REQUIRE(sums_out, ISO_ERR_INVALID, "iso_chamfer_nearest: null pointer");
  ISO_REQUIRE((x && idx_out) || p1 == 0, ISO_ERR_INVALID, "iso_chamfer_nearest: null pointer");
  ISO_REQUIRE((sorted_y && sorted_idx_y) || p2 == 0, ISO_ERR_INVALID, "iso_chamfer_nearest: null pointer");
  ISO_REQUIRE(off && grid_params, ISO_ERR_INVALID, "iso_chamfer_nearest: null pointer");
  ISO_REQUIRE((x_normals == nullptr) == (y_normals == nullptr), ISO_ERR_INVALID,
              "iso_chamfer_nearest: normals for both clouds or for neither");
  ISO_REQUIRE(workspace && workspace_bytes >= iso_chamfer_nearest_workspace_bytes(n_clouds, p1, p2), ISO_ERR_WORKSPACE,
              "iso_chamfer_nearest: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "iso_chamfer_nearest: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  float4* xyzi = reinterpret_cast<float4*>(workspace);
  float* partials = reinterpret_cast<float*>((char*)workspace + 16 * (int64_t)n_clouds * p2);
  const int gx = iso_capped_grid(p1, kNearBlock, kMaxPartials);
  pack_xyzi(sorted_y, sorted_idx_y, y_lengths, n_clouds, p2, xyzi, s);
  if (x_normals)
    hipLaunchKernelGGL(k_cham_nearest<true>, dim3(gx, n_clouds), dim3(kNearBlock), 0, s, x, x_lengths, xyzi, y_lengths, off,
                       grid_params, x_normals, y_normals, d2_out, idx_out, nterm_out, partials, p1, p2, g_stride);
  else
    hipLaunchKernelGGL(k_cham_nearest<false>, dim3(gx, n_clouds), dim3(kNearBlock), 0, s, x, x_lengths, xyzi, y_lengths, off,
                       grid_params, x_normals, y_normals, d2_out, idx_out, nterm_out, partials, p1, p2, g_stride);
  hipLaunchKernelGGL(k_cham_finish, dim3(n_clouds), dim3(128), 0, s, partials, gx, sums_out);
  ISO_CHECK_LAUNCH("iso_chamfer_nearest");
  return ISO_OK;
}

// workspace of iso_chamfer_backward: gather_lists.h's, with R = N * max(P1, P2) target rows and query rows per side
extern "C" int64_t iso_chamfer_backward_workspace_bytes(int n_clouds, int64_t p1, int64_t p2) {
  if (n_clouds < 0) n_clouds = 0;
  const int64_t pm = p1 > p2 ? (p1 > 0 ? p1 : 0) : (p2 > 0 ? p2 : 0);
  const int64_t R = (int64_t)n_clouds * pm;
  return gather_workspace_bytes(2 * R, 2 * R, pm, 2 * n_clouds);
}

extern "C" int iso_chamfer_backward(const float* x, const float* y, const int64_t* x_lengths, const int64_t* y_lengths,
                                    const int32_t* idx_x, const int32_t* idx_y, const float* g_dx, const float* g_dy,
                                    const float* x_normals, const float* y_normals, const float* g_nx, const float* g_ny,
                                    float* grad_x, float* grad_y, float* grad_x_normals, float* grad_y_normals,
                                    int n_clouds, int64_t p1, int64_t p2, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && p1 >= 0 && p2 >= 0, ISO_ERR_INVALID, "iso_chamfer_backward: bad sizes");
  const int64_t pm = p1 > p2 ? p1 : p2;
  ISO_REQUIRE((int64_t)n_clouds * pm < 0x7fffffff, ISO_ERR_UNSUPPORTED, "iso_chamfer_backward: 32-bit row indices");
  if (n_clouds == 0 || pm == 0 || (!grad_x && !grad_y)) return ISO_OK;
  ISO_REQUIRE(g_dx && g_dy && (p1 == 0 || (x && idx_x)) && (p2 == 0 || (y && idx_y)), ISO_ERR_INVALID,
              "iso_chamfer_backward: null pointer");
  ISO_REQUIRE((x_normals == nullptr) == (y_normals == nullptr), ISO_ERR_INVALID,
              "iso_chamfer_backward: normals for both clouds or for neither");
  ISO_REQUIRE((!grad_x_normals || grad_x) && (!grad_y_normals || grad_y), ISO_ERR_INVALID,
              "iso_chamfer_backward: a normal gradient needs its cloud's position gradient buffer");
  const bool normals = grad_x_normals || grad_y_normals;
  ISO_REQUIRE(!normals || (x_normals && g_nx && g_ny), ISO_ERR_INVALID, "iso_chamfer_backward: null pointer");
  ISO_REQUIRE(workspace && workspace_bytes >= iso_chamfer_backward_workspace_bytes(n_clouds, p1, p2), ISO_ERR_WORKSPACE,
              "iso_chamfer_backward: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "iso_chamfer_backward: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t R = (int64_t)n_clouds * pm;
  const GatherWorkspace w = gather_carve(workspace, 2 * R, 2 * R);   // every array [2][N][pm]
  Sides both;
  int ns = 0;
  auto lists = [&](const int32_t* idx_b, int64_t n_a, int64_t n_b) {
    return GatherView{idx_b, w.cnt + ns * R, w.off + ns * R, w.slot + ns * R, w.list + ns * R, n_b, n_a, n_b, pm};
  };
  if (grad_x && p1 > 0) {
    both.d[ns] = Side{x, y, x_normals, y_normals, x_lengths, idx_x, g_dx, g_dy, g_nx, g_ny, grad_x, grad_x_normals,
                      p1, p2, lists(idx_y, p1, p2), w.heavy + ns * R, w.heavy_count + ns};
    ++ns;
  }
  if (grad_y && p2 > 0) {
    both.d[ns] = Side{y, x, y_normals, x_normals, y_lengths, idx_y, g_dy, g_dx, g_ny, g_nx, grad_y, grad_y_normals,
                      p2, p1, lists(idx_x, p2, p1), w.heavy + ns * R, w.heavy_count + ns};
    ++ns;
  }
  if (ns == 0) return ISO_OK;
  if (ns == 1) both.d[1] = both.d[0];
  const int gm = iso_capped_grid(pm, 256, 4096);
  const int rc = gather_build(GatherViews{{both.d[0].lists, both.d[1].lists}}, ns, n_clouds, pm, w, 2 * R, pm,
                              2 * n_clouds, s);
  if (rc != ISO_OK) return rc;
  const int gh = (int)(R < 2048 ? R : 2048);
  if (normals) {
    hipLaunchKernelGGL(k_cham_grad<true>, dim3(gm, n_clouds, ns), dim3(256), 0, s, both);
    hipLaunchKernelGGL(k_cham_grad_heavy<true>, dim3(gh, 1, ns), dim3(64), 0, s, both);
  } else {
    hipLaunchKernelGGL(k_cham_grad<false>, dim3(gm, n_clouds, ns), dim3(256), 0, s, both);
    hipLaunchKernelGGL(k_cham_grad_heavy<false>, dim3(gh, 1, ns), dim3(64), 0, s, both);
  }
  ISO_CHECK_LAUNCH("iso_chamfer_backward");
  return ISO_OK;
}
