// The sign of the point-to-mesh distance by angle-weighted pseudonormals (Baerentzen & Aanaes), written for gfx950.
// Stands in for the inside test of the reference's SignedDistanceLoss (include/isopoints.h section J for the call site).
//
//   k_ps_faces        : per face the unit normal (zero for a face without area), its three corner angles and, for the
//                       gather, the vertex each of its three corners chose
//   k_ps_vertex       : one lane per vertex: sum of angle * normal over its corners, a list of up to kLightList corners in
//                       ascending corner order; a longer list is left to
//   k_ps_vertex_heavy : one wave per long list (gather_wave), the 64 lanes' sums added by one butterfly
//   k_ps_edges        : one lane per (face, slot): the sum of the normals of all faces that hold both end vertices of the
//                       edge, in ascending face order, found on the corner list of the end vertex with the shorter list
//   k_ps_sign         : one lane per point: pf_closest() against the nearest face the search wrote, the feature from the
//                       weights that are exactly zero, the sign of (p - c) . N
//
// The corner lists are gather_lists.h's (query = corner, target = vertex, one flat cloud): integer atomics only, and every
// sum runs in a fixed order, so two runs give the same bits.
#include <float.h>
#include "gather_lists.h"
#include "pf_closest.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPsBlock = 256;

// 0 = face interior, 1..3 = edge slot + 1 (slot k: vertex k -> vertex k + 1 mod 3), 4..6 = corner + 4; by the weights of
// the closest point that are exactly zero
__host__ __device__ __forceinline__ int ps_feature(const float (&bw)[3]) {
  const bool z0 = bw[0] == 0.f, z1 = bw[1] == 0.f, z2 = bw[2] == 0.f;
  const int zeros = (z0 ? 1 : 0) + (z1 ? 1 : 0) + (z2 ? 1 : 0);
  if (zeros == 1) return z0 ? 2 : (z1 ? 3 : 1);        // the edge opposite the vertex without weight
  if (zeros == 2) return !z0 ? 4 : (!z1 ? 5 : 6);      // the vertex that keeps its weight
  return 0;
}

__device__ __forceinline__ void ps_sub(const float* a, const float* b, float (&o)[3]) {
  o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2];
}
__device__ __forceinline__ void ps_cross(const float (&x)[3], const float (&y)[3], float (&o)[3]) {
  o[0] = x[1] * y[2] - x[2] * y[1];
  o[1] = x[2] * y[0] - x[0] * y[2];
  o[2] = x[0] * y[1] - x[1] * y[0];
}
__device__ __forceinline__ float ps_dot(const float (&x)[3], const float (&y)[3]) {
  return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// the three packed vertex rows of face f; false where one lies outside [0, n_verts)
__device__ __forceinline__ bool ps_face_rows(const int64_t* __restrict__ faces, int64_t f, int64_t n_verts, int64_t (&r)[3]) {
  r[0] = faces[f * 3]; r[1] = faces[f * 3 + 1]; r[2] = faces[f * 3 + 2];
  return r[0] >= 0 && r[0] < n_verts && r[1] >= 0 && r[1] < n_verts && r[2] >= 0 && r[2] < n_verts;
}

// ---- faces ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPsBlock) void k_ps_faces(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                       int64_t n_verts, int64_t n_faces, float* __restrict__ face_normals,
                                                       float* __restrict__ angles, int32_t* __restrict__ corner_vertex) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * blockDim.x) {
    int64_t r[3];
    float n[3] = {0.f, 0.f, 0.f}, ang[3] = {0.f, 0.f, 0.f};
    const bool ok = ps_face_rows(faces, f, n_verts, r);
    if (ok) {
      float v[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] = verts[r[k] * 3 + c];
      }
      float e1[3], e2[3], m[3];
      ps_sub(v[1], v[0], e1);
      ps_sub(v[2], v[0], e2);
      ps_cross(e1, e2, m);
      const float len = sqrtf(ps_dot(m, m));
      if (len > 0.f && len <= FLT_MAX) {   // a face without area (or with a NaN one) contributes nothing anywhere
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = m[c] / len;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float a[3], b[3], x[3];
          ps_sub(v[(k + 1) % 3], v[k], a);
          ps_sub(v[(k + 2) % 3], v[k], b);
          ps_cross(a, b, x);
          ang[k] = atan2f(sqrtf(ps_dot(x, x)), ps_dot(a, b));
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      face_normals[f * 3 + c] = n[c];
      angles[f * 3 + c] = ang[c];
      corner_vertex[f * 3 + c] = ok ? (int32_t)r[c] : -1;
    }
  }
}

// ---- vertices ---------------------------------------------------------------------------------------------------
struct PsVerts {
  const float* face_normals;   // (F,3)
  const float* angles;         // (3F)
  float* vert_normals;         // (V,3)
  int64_t n_verts;
  GatherView lists;            // one cloud: idx (3F) = the vertex of each corner
  int32_t* heavy;              // (V)
  int32_t* heavy_count;
};

__device__ __forceinline__ void ps_add_corner(const PsVerts& a, int64_t c, float (&acc)[3]) {
  const float w = a.angles[c];
  const int64_t f = c / 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] += w * a.face_normals[f * 3 + k];
}

__global__ __launch_bounds__(kPsBlock) void k_ps_vertex(PsVerts a) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_verts; i += (int64_t)gridDim.x * blockDim.x) {
    float acc[3] = {0.f, 0.f, 0.f};
    const int L = a.lists.cnt[i];
    if (L > kLightList) {
      a.heavy[atomicAdd(a.heavy_count, 1)] = (int32_t)i;   // the order of this list decides nothing: one wave per entry
      continue;                                            // k_ps_vertex_heavy writes this vertex
    }
    if (L > 0) gather_lane(gather_list(a.lists, 0, i), L, [&](int c) { ps_add_corner(a, c, acc); });
#pragma unroll
    for (int k = 0; k < 3; ++k) a.vert_normals[i * 3 + k] = acc[k];
  }
}

__global__ __launch_bounds__(64) void k_ps_vertex_heavy(PsVerts a) {
  __shared__ int32_t s_raw[kSortList], s_sorted[kSortList];
  const int lane = threadIdx.x;
  const int count = *a.heavy_count;
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int i = a.heavy[w];
    const int L = a.lists.cnt[i];
    float acc[3] = {0.f, 0.f, 0.f};
    gather_wave(a.lists, 0, i, L, lane, s_raw, s_sorted, [&](int64_t c) { ps_add_corner(a, c, acc); });
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = iso_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) a.vert_normals[(int64_t)i * 3 + k] = acc[k];
    }
  }
}

// ---- edges ------------------------------------------------------------------------------------------------------
// Slot k of face f: the edge from its vertex k to its vertex k + 1 mod 3.  Every face that holds both end vertices has a
// corner on the list of either; the lane walks the shorter of the two lists and takes the faces that also hold the other
// end, the smallest face index above the last one taken each time: ascending face order whatever order the list has.
__global__ __launch_bounds__(kPsBlock) void k_ps_edges(const int64_t* __restrict__ faces, const float* __restrict__ face_normals,
                                                       GatherView lists, int64_t n_verts, int64_t n_faces,
                                                       float* __restrict__ edge_normals) {
  const int64_t n_slots = n_faces * 3;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_slots; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = e / 3;
    const int k = (int)(e - f * 3);
    int64_t r[3];
    float acc[3] = {0.f, 0.f, 0.f};
    const bool ok = ps_face_rows(faces, f, n_verts, r);
    int64_t a = k == 0 ? r[0] : (k == 1 ? r[1] : r[2]);        // selects: a dynamic index would put r in scratch or LDS
    int64_t b = k == 0 ? r[1] : (k == 1 ? r[2] : r[0]);
    if (ok && a != b) {
      if (lists.cnt[b] < lists.cnt[a]) { const int64_t t = a; a = b; b = t; }
      const int L = lists.cnt[a];
      const int32_t* li = gather_list(lists, 0, a);
      int64_t last = -1;
      for (;;) {
        int64_t nxt = n_faces;
        for (int m = 0; m < L; ++m) {
          const int64_t g = li[m] / 3;
          if (g <= last || g >= nxt) continue;
          if (faces[g * 3] == b || faces[g * 3 + 1] == b || faces[g * 3 + 2] == b) nxt = g;
        }
        if (nxt >= n_faces) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += face_normals[nxt * 3 + c];
        last = nxt;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) edge_normals[e * 3 + c] = acc[c];
  }
}

// ---- the sign ---------------------------------------------------------------------------------------------------
struct PsSign {
  const float* points;         // (P,3)
  const int32_t* idx;          // (P) the packed nearest face, -1 = none
  const float* tris;           // (F,9)
  const int64_t* faces;        // (F,3)
  const float* face_normals;   // (F,3)
  const float* edge_normals;   // (F,9)
  const float* vert_normals;   // (V,3)
  float* sign_out;             // (P)
  int32_t* feature_out;        // (P)
  int64_t n_points, n_faces, n_verts;
  float min_area;
};

__global__ __launch_bounds__(kPsBlock) void k_ps_sign(PsSign a) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.n_points; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = a.idx[q];
    float sign = 1.0f;
    int feature = -1;
    if (f >= 0 && f < a.n_faces) {
      float p[3], v[9], bw[3], N[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = a.points[q * 3 + c];
#pragma unroll
      for (int c = 0; c < 9; ++c) v[c] = a.tris[f * 9 + c];
      pf_closest(p, v, a.min_area, bw);
      feature = ps_feature(bw);
      const float* src = nullptr;
      if (feature == 0) {
        src = a.face_normals + f * 3;
      } else if (feature <= 3) {
        src = a.edge_normals + f * 9 + (feature - 1) * 3;
      } else {
        const int64_t row = a.faces[f * 3 + (feature - 4)];
        if (row >= 0 && row < a.n_verts) src = a.vert_normals + row * 3;
      }
      if (src) { N[0] = src[0]; N[1] = src[1]; N[2] = src[2]; }
      float r[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = p[c] - ((bw[0] * v[c] + bw[1] * v[3 + c]) + bw[2] * v[6 + c]);
      if (ps_dot(r, N) < 0.f) sign = -1.0f;
    }
    a.sign_out[q] = sign;
    a.feature_out[q] = feature;
  }
}

// workspace of iso_pfsign_normals: [corner -> vertex: 3F ints][corner angles: 3F floats][gather_lists.h's, V target rows
// and 3F query rows]
inline int64_t ps_corner_bytes(int64_t n_faces) { return iso_align16(12 * n_faces); }

}  // namespace

extern "C" int64_t iso_pfsign_normals_workspace_bytes(int64_t n_verts, int64_t n_faces) {
  if (n_verts < 0) n_verts = 0;
  if (n_faces < 0) n_faces = 0;
  return 2 * ps_corner_bytes(n_faces) + gather_workspace_bytes(n_verts, 3 * n_faces, n_verts, 1);
}

extern "C" int iso_pfsign_normals(const float* verts, const int64_t* faces, int64_t n_verts, int64_t n_faces,
                                  float* face_normals_out, float* edge_normals_out, float* vert_normals_out,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(n_verts >= 0 && n_faces >= 0, ISO_ERR_INVALID, "iso_pfsign_normals: bad sizes");
  ISO_REQUIRE(n_verts < 0x7fffffff && n_faces < 0x7fffffff / 3, ISO_ERR_UNSUPPORTED,
              "iso_pfsign_normals: 32-bit indices (V < 2^31, 3 F < 2^31)");
  if (n_verts == 0 && n_faces == 0) return ISO_OK;
  ISO_REQUIRE((n_faces == 0 || (faces && face_normals_out && edge_normals_out)) && (n_verts == 0 || (verts && vert_normals_out)),
              ISO_ERR_INVALID, "iso_pfsign_normals: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_faces == 0 || n_verts == 0) {
    // no face reaches a vertex: every vector is zero
    if (n_verts > 0) iso_zero_words(vert_normals_out, n_verts * 3, s);
    if (n_faces > 0) {
      iso_zero_words(face_normals_out, n_faces * 3, s);
      iso_zero_words(edge_normals_out, n_faces * 9, s);
    }
    ISO_CHECK_LAUNCH("iso_pfsign_normals");
    return ISO_OK;
  }
  ISO_REQUIRE(workspace && workspace_bytes >= iso_pfsign_normals_workspace_bytes(n_verts, n_faces), ISO_ERR_WORKSPACE,
              "iso_pfsign_normals: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "iso_pfsign_normals: workspace must be 16-B aligned");
  const int64_t n_corners = 3 * n_faces;
  int32_t* corner_vertex = reinterpret_cast<int32_t*>(workspace);
  float* angles = reinterpret_cast<float*>((char*)workspace + ps_corner_bytes(n_faces));
  const GatherWorkspace w = gather_carve((char*)workspace + 2 * ps_corner_bytes(n_faces), n_verts, n_corners);
  const GatherView lists{corner_vertex, w.cnt, w.off, w.slot, w.list, n_corners, n_verts, n_corners, n_verts};
  hipLaunchKernelGGL(k_ps_faces, dim3(iso_capped_grid(n_faces, kPsBlock, 4096)), dim3(kPsBlock), 0, s, verts, faces, n_verts,
                     n_faces, face_normals_out, angles, corner_vertex);
  const int rc = gather_build(GatherViews{{lists, lists}}, 1, 1, n_corners, w, n_verts, n_verts, 1, s);
  if (rc != ISO_OK) return rc;
  PsVerts a{face_normals_out, angles, vert_normals_out, n_verts, lists, w.heavy, w.heavy_count};
  hipLaunchKernelGGL(k_ps_vertex, dim3(iso_capped_grid(n_verts, kPsBlock, 4096)), dim3(kPsBlock), 0, s, a);
  hipLaunchKernelGGL(k_ps_vertex_heavy, dim3((int)(n_verts < 2048 ? n_verts : 2048)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_ps_edges, dim3(iso_capped_grid(n_corners, kPsBlock, 4096)), dim3(kPsBlock), 0, s, faces,
                     (const float*)face_normals_out, lists, n_verts, n_faces, edge_normals_out);
  ISO_CHECK_LAUNCH("iso_pfsign_normals");
  return ISO_OK;
}

extern "C" int iso_pfsign_sign(const float* points, const int32_t* idx, const float* tris, const int64_t* faces,
                               const float* face_normals, const float* edge_normals, const float* vert_normals,
                               float min_triangle_area, float* sign_out, int32_t* feature_out, int64_t n_points,
                               int64_t n_faces, int64_t n_verts, void* stream) {
  ISO_REQUIRE(n_points >= 0 && n_faces >= 0 && n_verts >= 0, ISO_ERR_INVALID, "iso_pfsign_sign: bad sizes");
  ISO_REQUIRE(n_points < 0x7fffffff && n_verts < 0x7fffffff && n_faces < 0x7fffffff / 3, ISO_ERR_UNSUPPORTED,
              "iso_pfsign_sign: 32-bit indices (P < 2^31, V < 2^31, 3 F < 2^31)");
  ISO_REQUIRE(min_triangle_area >= 0.f, ISO_ERR_INVALID, "iso_pfsign_sign: min_triangle_area is negative");
  if (n_points == 0) return ISO_OK;
  ISO_REQUIRE(points && idx && sign_out && feature_out, ISO_ERR_INVALID, "iso_pfsign_sign: null pointer");
  ISO_REQUIRE(n_faces == 0 || (tris && faces && face_normals && edge_normals), ISO_ERR_INVALID,
              "iso_pfsign_sign: null pointer");
  ISO_REQUIRE(n_verts == 0 || vert_normals, ISO_ERR_INVALID, "iso_pfsign_sign: null pointer");
  PsSign a{points, idx, tris, faces, face_normals, edge_normals, vert_normals, sign_out, feature_out,
           n_points, n_faces, n_verts, min_triangle_area};
  hipLaunchKernelGGL(k_ps_sign, dim3(iso_capped_grid(n_points, kPsBlock, 4096)), dim3(kPsBlock), 0, (hipStream_t)stream, a);
  ISO_CHECK_LAUNCH("iso_pfsign_sign");
  return ISO_OK;
}

extern "C" int iso_pfsign_pair(const float* point, const float* tri, float min_triangle_area, float* d2_out,
                               float* weights_out, int32_t* feature_out) {
  ISO_REQUIRE(point && tri && d2_out && weights_out && feature_out, ISO_ERR_INVALID, "iso_pfsign_pair: null pointer");
  ISO_REQUIRE(min_triangle_area >= 0.f, ISO_ERR_INVALID, "iso_pfsign_pair: min_triangle_area is negative");
  float p[3], v[9], bw[3];
  for (int c = 0; c < 3; ++c) p[c] = point[c];
  for (int c = 0; c < 9; ++c) v[c] = tri[c];
  *d2_out = pf_closest(p, v, min_triangle_area, bw);
  for (int c = 0; c < 3; ++c) weights_out[c] = bw[c];
  *feature_out = ps_feature(bw);
  return ISO_OK;
}
