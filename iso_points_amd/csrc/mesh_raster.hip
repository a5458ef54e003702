// Triangle-mesh rasterisation for gfx950: per pixel the K nearest faces with depth, barycentric coordinates and the
// (negative) squared distance to the face's outline -- pytorch3d.renderer.mesh.rasterize_meshes at blur_radius = 0, the
// only way the reference calls it (include/isopoints.h section M has the rule and the call sites).
//
// The splat raster's skeleton (splat_raster.hip) and its K-best list (kbest.h) with another inside test: faces are
// binned into 16x16-pixel tiles by a count -> iso_splat_tile_offsets -> fill counting sort over their clamped bounding
// boxes (integer atomics only), and one
// 256-lane workgroup per tile streams the tile's face list through LDS in 256-face chunks -- every lane reads the same
// LDS words, a broadcast -- while each lane keeps the K nearest (pz, face) pairs of its own pixel in registers.  The
// order of a tile's list is whatever the fill's atomics made it; the K-best rule is the total order (pz, face index), so
// the result does not depend on it.  A face list has no capacity: the pair list is allocated at the counted size.
//
// Every expression of the rule (face_setup, the edge functions, pair_depth, seg_dist2) is written in the order the float32
// restatement of tests/mesh_raster_oracle.py writes it, with FMA contraction off and IEEE division: the kernel and that
// restatement compute the same bits.  Two things follow from "exactly the rule":
//   * the quotients w_i = edge_i / area are divisions, not products with a staged 1 / area (one more rounding would leave
//     the restatement); they run only for the pixels whose three edge functions are non-zero and of the area's sign, a
//     necessary condition of w_i > 0 that costs three compares;
//   * the list holds (pz, id) only.  Barycentrics and the outline distance are recomputed for the K survivors from the
//     face's vertices in the epilogue -- the same instructions on the same operands.
#include <float.h>
#include "iso_common.h"
#include "kbest.h"

#pragma clang fp contract(off)

namespace {

constexpr int MTILE = 16;        // pixels per tile side (iso_splat_tiles_per_side's)
constexpr int MCHUNK = 256;      // faces staged per pass through LDS

// edge(a, b; q) = (qx - ax)(by - ay) - (qy - ay)(bx - ax), in this difference form
__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float qx, float qy) {
  return (qx - ax) * (by - ay) - (qy - ay) * (bx - ax);
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }   // false for NaN and +-inf

// pixel centre of output column / row i on a side of S pixels (pytorch3d's PixToNdc with its flip)
__device__ __forceinline__ float pix_centre(int i, int S) { return 1.0f - (float)(2 * i + 1) / (float)S; }

// Output columns (or rows) whose centre can lie in [lo, hi] of NDC, one pixel of slack on either side, clamped to the
// image.  The inside test is strict, so a covered centre lies strictly inside the face's box.
__device__ __forceinline__ bool centre_range(float lo, float hi, int S, int& i0, int& i1) {
  float f0 = ((1.0f - hi) * (float)S - 1.0f) * 0.5f;
  float f1 = ((1.0f - lo) * (float)S - 1.0f) * 0.5f;
  if (!(f0 < 1e9f) || !(f1 > -1e9f)) return false;
  f0 = fmaxf(f0, -4.0f);
  f1 = fminf(f1, (float)S + 4.0f);
  i0 = (int)ceilf(f0) - 1;
  i1 = (int)floorf(f1) + 1;
  if (i0 < 0) i0 = 0;
  if (i1 > S - 1) i1 = S - 1;
  return i0 <= i1;
}

// The skip test of the rule and the face's pixel box.  v: nine floats (x, y, z of v0, v1, v2).
__device__ __forceinline__ bool face_setup(const float* __restrict__ v, int S, int cull, int& c0, int& c1, int& r0, int& r1) {
  const float x0 = v[0], y0 = v[1], z0 = v[2], x1 = v[3], y1 = v[4], z1 = v[5], x2 = v[6], y2 = v[7], z2 = v[8];
  const bool fin = finite_f(x0) && finite_f(y0) && finite_f(z0) && finite_f(x1) && finite_f(y1) && finite_f(z1) &&
                   finite_f(x2) && finite_f(y2) && finite_f(z2);
  if (!fin) return false;
  const float area = edge_fn(x0, y0, x1, y1, x2, y2);
  if (!(fabsf(area) > 1e-8f)) return false;
  if (fmaxf(fmaxf(z0, z1), z2) < 0.0f) return false;
  if (cull && area < 0.0f) return false;
  return centre_range(fminf(fminf(x0, x1), x2), fmaxf(fmaxf(x0, x1), x2), S, c0, c1) &&
         centre_range(fminf(fminf(y0, y1), y2), fmaxf(fmaxf(y0, y1), y2), S, r0, r1);
}

// mesh of packed face f: the last n with first[n] <= f (first is non-decreasing: packed order), or -1 when f lies
// outside that mesh's faces
__device__ __forceinline__ int mesh_of_face(const int64_t* __restrict__ first, const int64_t* __restrict__ num, int N, int64_t f) {
  int lo = 0, hi = N;              // first[lo - 1] <= f < first[hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= f) lo = mid + 1; else hi = mid;
  }
  const int n = lo - 1;
  return (n >= 0 && f < first[n] + num[n]) ? n : -1;
}

// count (FILL = false) and fill (FILL = true): one lane per packed face, the same walk
template <bool FILL>
__global__ __launch_bounds__(256) void k_mesh_bin(const float* __restrict__ face_verts, const int64_t* __restrict__ first,
                                                  const int64_t* __restrict__ num, int N, int64_t F, int S, int T, int cull,
                                                  int32_t* __restrict__ tile_cnt, const int32_t* __restrict__ tile_off,
                                                  int32_t* __restrict__ pairs, int64_t capacity) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    const int n = mesh_of_face(first, num, N, f);
    if (n < 0) continue;
    int c0, c1, r0, r1;
    if (!face_setup(face_verts + f * 9, S, cull, c0, c1, r0, r1)) continue;
    for (int ty = r0 / MTILE; ty <= r1 / MTILE; ++ty)
      for (int tx = c0 / MTILE; tx <= c1 / MTILE; ++tx) {
        const int tile = (n * T + ty) * T + tx;
        const int slot = atomicAdd(&tile_cnt[tile], 1);
        if (FILL) {
          const int64_t dst = (int64_t)tile_off[tile] + slot;
          if (dst >= 0 && dst < capacity) pairs[dst] = (int32_t)f;
        }
      }
  }
}

// w -> b -> pz of an inside pixel (e_i the edge functions, already of the area's sign).  false: the pair is skipped.
__device__ __forceinline__ bool pair_depth(float e0, float e1, float e2, float area, float z0, float z1, float z2, int persp,
                                           float& b0, float& b1, float& b2, float& pz) {
  const float w0 = e0 / area, w1 = e1 / area, w2 = e2 / area;
  if (!(w0 > 0.0f && w1 > 0.0f && w2 > 0.0f)) return false;
  b0 = w0; b1 = w1; b2 = w2;
  if (persp) {
    const float t0 = w0 * z1 * z2, t1 = w1 * z0 * z2, t2 = w2 * z0 * z1;
    const float den = (t0 + t1) + t2;
    b0 = t0 / den; b1 = t1 / den; b2 = t2 / den;
  }
  pz = (b0 * z0 + b1 * z1) + b2 * z2;
  return pz >= 0.0f && finite_f(pz);
}

// squared distance in NDC xy from p to segment (a, b) -- pytorch3d's PointLineDistanceForward
__device__ __forceinline__ float seg_dist2(float px, float py, float ax, float ay, float bx, float by) {
  const float dx = bx - ax, dy = by - ay;
  const float l2 = dx * dx + dy * dy;
  if (l2 <= 1e-8f) { const float qx = px - bx, qy = py - by; return qx * qx + qy * qy; }
  float t = (dx * (px - ax) + dy * (py - ay)) / l2;
  t = fminf(fmaxf(t, 0.0f), 1.0f);
  const float qx = px - (ax + t * dx), qy = py - (ay + t * dy);
  return qx * qx + qy * qy;
}

template <int KMAX>
__global__ __launch_bounds__(256) void k_mesh_raster(const float* __restrict__ face_verts, int64_t n_faces,
                                                     const int32_t* __restrict__ tile_off,
                                                     const int32_t* __restrict__ pairs, int64_t capacity, int S, int T, int K,
                                                     int persp, int64_t* __restrict__ pix_to_face, float* __restrict__ zbuf,
                                                     float* __restrict__ bary, float* __restrict__ dists) {
  // one chunk of faces, SoA in float4 so that a pixel thread takes a face in five broadcast reads
  __shared__ float4 s_p01[MCHUNK];   // x0, y0, x1, y1
  __shared__ float4 s_p2[MCHUNK];    // x2, y2, area, id
  __shared__ float4 s_d0[MCHUNK];    // y2 - y1, x2 - x1, y0 - y2, x0 - x2
  __shared__ float4 s_d1[MCHUNK];    // y1 - y0, x1 - x0, -, -
  __shared__ float4 s_z[MCHUNK];     // z0, z1, z2, -
  const int tile = blockIdx.x;
  const int tx = tile % T, ty = (tile / T) % T, n = tile / (T * T);
  const int lx = threadIdx.x % MTILE, ly = threadIdx.x / MTILE;
  const int c = tx * MTILE + lx, r = ty * MTILE + ly;
  const bool in_image = c < S && r < S;
  const float px = pix_centre(c, S), py = pix_centre(r, S);
  KBest<KMAX, false> best;           // the K nearest (pz, face): depths are >= +0 and never NaN (pair_depth, then + 0.0f)
  best.init();
  const int64_t off = tile_off[tile];
  int cnt = tile_off[tile + 1] - tile_off[tile];
  if (off < 0 || cnt < 0) cnt = 0;
  if (off + cnt > capacity) cnt = off < capacity ? (int)(capacity - off) : 0;
  for (int c0 = 0; c0 < cnt; c0 += MCHUNK) {
    const int m = min(MCHUNK, cnt - c0);
    __syncthreads();                                   // the previous chunk has been read
    if ((int)threadIdx.x < m) {
      const int f = pairs[off + c0 + threadIdx.x];
      // (a list entry is a face the fill pass wrote; one outside [0, F) is staged as a face no pixel is inside of)
      const bool valid = f >= 0 && (int64_t)f < n_faces;
      const float* v = face_verts + (valid ? (int64_t)f * 9 : 0);
      const float x0 = v[0], y0 = v[1], x1 = v[3], y1 = v[4], x2 = v[6], y2 = v[7];
      s_p01[threadIdx.x] = make_float4(x0, y0, x1, y1);
      s_p2[threadIdx.x] = make_float4(x2, y2, valid ? edge_fn(x0, y0, x1, y1, x2, y2) : __int_as_float(0x7fc00000),
                                      __int_as_float(f));
      s_d0[threadIdx.x] = make_float4(y2 - y1, x2 - x1, y0 - y2, x0 - x2);
      s_d1[threadIdx.x] = make_float4(y1 - y0, x1 - x0, 0.0f, 0.0f);
      s_z[threadIdx.x] = make_float4(v[2], v[5], v[8], 0.0f);
    }
    __syncthreads();
    if (in_image) {
      for (int k = 0; k < m; ++k) {
        const float4 a = s_p01[k], b = s_p2[k], d0 = s_d0[k], d1 = s_d1[k];
        const float area = b.z;
        // edge(v1, v2; p), edge(v2, v0; p), edge(v0, v1; p)
        const float e0 = (px - a.z) * d0.x - (py - a.w) * d0.y;
        const float e1 = (px - b.x) * d0.z - (py - b.y) * d0.w;
        const float e2 = (px - a.x) * d1.x - (py - a.y) * d1.y;
        // w_i = e_i / area > 0 needs e_i != 0 of the area's sign: three compares decide most pairs, no division
        const bool neg = area < 0.0f;
        if (!((neg ? e0 < 0.0f : e0 > 0.0f) & (neg ? e1 < 0.0f : e1 > 0.0f) & (neg ? e2 < 0.0f : e2 > 0.0f))) continue;
        const float4 z = s_z[k];
        float b0, b1, b2, pz;
        if (!pair_depth(e0, e1, e2, area, z.x, z.y, z.z, persp, b0, b1, b2, pz)) continue;
        pz += 0.0f;                                    // -0 -> +0: push_masked orders depths by their bit patterns
        const int id = __float_as_int(b.w);
        if (pz < best.z[KMAX - 1] || (pz == best.z[KMAX - 1] && id < best.id[KMAX - 1])) best.push_masked(pz, id, KMAX);
      }
    }
  }
  if (!in_image) return;
  // the K survivors: barycentrics and outline distance from the face's own vertices, the same expressions
  const int64_t pix = ((int64_t)n * S + r) * S + c;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < K) {
      const int64_t o = pix * K + j;
      const int id = best.id[j];
      if (id == 0x7fffffff) {
        pix_to_face[o] = -1; zbuf[o] = -1.0f; dists[o] = -1.0f;
        bary[o * 3] = -1.0f; bary[o * 3 + 1] = -1.0f; bary[o * 3 + 2] = -1.0f;
      } else {
        const float* v = face_verts + (int64_t)id * 9;
        const float x0 = v[0], y0 = v[1], z0 = v[2], x1 = v[3], y1 = v[4], z1 = v[5], x2 = v[6], y2 = v[7], z2 = v[8];
        const float area = edge_fn(x0, y0, x1, y1, x2, y2);
        const float e0 = (px - x1) * (y2 - y1) - (py - y1) * (x2 - x1);
        const float e1 = (px - x2) * (y0 - y2) - (py - y2) * (x0 - x2);
        const float e2 = (px - x0) * (y1 - y0) - (py - y0) * (x1 - x0);
        float b0 = -1.0f, b1 = -1.0f, b2 = -1.0f, pz = -1.0f;
        pair_depth(e0, e1, e2, area, z0, z1, z2, persp, b0, b1, b2, pz);
        const float d = fminf(fminf(seg_dist2(px, py, x0, y0, x1, y1), seg_dist2(px, py, x0, y0, x2, y2)),
                              seg_dist2(px, py, x1, y1, x2, y2));
        pix_to_face[o] = id; zbuf[o] = best.z[j]; dists[o] = -d;
        bary[o * 3] = b0; bary[o * 3 + 1] = b1; bary[o * 3 + 2] = b2;
      }
    }
  }
}

// what every entry refuses (nothing is launched): returns 0 when the sizes are acceptable
int check_sizes(const char* fn, int n_meshes, int64_t n_faces, int S, int K) {
  ISO_REQUIRE(n_meshes >= 0 && n_faces >= 0, ISO_ERR_INVALID, "%s: negative size (n_meshes %d, n_faces %lld)", fn, n_meshes,
              (long long)n_faces);
  ISO_REQUIRE(S >= 1, ISO_ERR_INVALID, "%s: image_size %d must be at least 1", fn, S);
  ISO_REQUIRE(K >= 1 && K <= 8, ISO_ERR_INVALID, "%s: faces_per_pixel %d is outside 1..8", fn, K);
  ISO_REQUIRE(n_faces < ((int64_t)1 << 31), ISO_ERR_INVALID, "%s: %lld packed faces; the limit is 2^31 - 1", fn,
              (long long)n_faces);
  // in double first: n * S * S * K may not fit 64 bits
  ISO_REQUIRE((double)n_meshes * (double)S * (double)S * (double)K < 2147483648.0, ISO_ERR_INVALID,
              "%s: n_meshes * image_size^2 * faces_per_pixel = %d * %d^2 * %d; the limit is 2^31 - 1", fn, n_meshes, S, K);
  return ISO_OK;
}

int bin_grid(int64_t F) {
  int64_t g = (F + 255) / 256;
  if (g > 8192) g = 8192;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

extern "C" int iso_meshraster_form(int faces_per_pixel) {
  const int K = faces_per_pixel;
  return K < 1 || K > 8 ? 0 : (K == 1 ? 1 : (K <= 4 ? 4 : 8));
}

extern "C" int iso_meshraster_count(const float* face_verts, const int64_t* first_idx, const int64_t* num_faces, int n_meshes,
                                     int64_t n_faces, int image_size, int cull_backfaces, int32_t* tile_cnt, void* stream) {
  const char* fn = "iso_meshraster_count";
  if (int rc = check_sizes(fn, n_meshes, n_faces, image_size, 1)) return rc;
  if (n_meshes == 0 || n_faces == 0) return ISO_OK;
  ISO_REQUIRE(face_verts && first_idx && num_faces && tile_cnt, ISO_ERR_INVALID, "%s: null pointer", fn);
  const int T = (image_size + MTILE - 1) / MTILE;
  hipLaunchKernelGGL(k_mesh_bin<false>, dim3(bin_grid(n_faces)), dim3(256), 0, (hipStream_t)stream, face_verts, first_idx,
                     num_faces, n_meshes, n_faces, image_size, T, cull_backfaces ? 1 : 0, tile_cnt, nullptr, nullptr,
                     (int64_t)0);
  ISO_CHECK_LAUNCH(fn);
  return ISO_OK;
}

extern "C" int iso_meshraster_fill(const float* face_verts, const int64_t* first_idx, const int64_t* num_faces, int n_meshes,
                                    int64_t n_faces, int image_size, int cull_backfaces, int32_t* tile_cursor,
                                    const int32_t* tile_off, int32_t* pairs, int64_t pair_capacity, void* stream) {
  const char* fn = "iso_meshraster_fill";
  if (int rc = check_sizes(fn, n_meshes, n_faces, image_size, 1)) return rc;
  ISO_REQUIRE(pair_capacity >= 0, ISO_ERR_INVALID, "%s: negative pair_capacity", fn);
  if (n_meshes == 0 || n_faces == 0 || pair_capacity == 0) return ISO_OK;
  ISO_REQUIRE(face_verts && first_idx && num_faces && tile_cursor && tile_off && pairs, ISO_ERR_INVALID, "%s: null pointer", fn);
  const int T = (image_size + MTILE - 1) / MTILE;
  hipLaunchKernelGGL(k_mesh_bin<true>, dim3(bin_grid(n_faces)), dim3(256), 0, (hipStream_t)stream, face_verts, first_idx,
                     num_faces, n_meshes, n_faces, image_size, T, cull_backfaces ? 1 : 0, tile_cursor, tile_off, pairs,
                     pair_capacity);
  ISO_CHECK_LAUNCH(fn);
  return ISO_OK;
}

extern "C" int iso_meshraster_pixels(const float* face_verts, int n_meshes, int64_t n_faces, int image_size,
                                      int faces_per_pixel, int perspective_correct, const int32_t* tile_off,
                                      const int32_t* pairs, int64_t pair_capacity, int64_t* pix_to_face, float* zbuf,
                                      float* bary, float* dists, void* stream) {
  const char* fn = "iso_meshraster_pixels";
  if (int rc = check_sizes(fn, n_meshes, n_faces, image_size, faces_per_pixel)) return rc;
  ISO_REQUIRE(pair_capacity >= 0, ISO_ERR_INVALID, "%s: negative pair_capacity", fn);
  if (n_meshes == 0) return ISO_OK;
  ISO_REQUIRE(tile_off && pix_to_face && zbuf && bary && dists, ISO_ERR_INVALID, "%s: null pointer", fn);
  ISO_REQUIRE(pair_capacity == 0 || (pairs && face_verts), ISO_ERR_INVALID, "%s: null pointer", fn);
  const int S = image_size, K = faces_per_pixel, persp = perspective_correct ? 1 : 0;
  const int T = (S + MTILE - 1) / MTILE;
  const dim3 grid(n_meshes * T * T), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (iso_meshraster_form(K)) {
    case 1:
      hipLaunchKernelGGL(k_mesh_raster<1>, grid, block, 0, s, face_verts, n_faces, tile_off, pairs, pair_capacity, S, T, K, persp,
                         pix_to_face, zbuf, bary, dists);
      break;
    case 4:
      hipLaunchKernelGGL(k_mesh_raster<4>, grid, block, 0, s, face_verts, n_faces, tile_off, pairs, pair_capacity, S, T, K, persp,
                         pix_to_face, zbuf, bary, dists);
      break;
    default:
      hipLaunchKernelGGL(k_mesh_raster<8>, grid, block, 0, s, face_verts, n_faces, tile_off, pairs, pair_capacity, S, T, K, persp,
                         pix_to_face, zbuf, bary, dists);
      break;
  }
  ISO_CHECK_LAUNCH(fn);
  return ISO_OK;
}
