// Area-weighted sampling of points and normals on packed triangle meshes, written for gfx950.  Stands in for
// pytorch3d.ops.sample_points_from_meshes as the reference calls it (include/isopoints.h section I for the call sites).
//
//   k_mesh_areas      : per face the float32 area and unit normal
//   k_mesh_scan_tiles : per mesh and tile of 2048 faces the inclusive running sum of the areas in float64, local to the tile
//   k_mesh_scan_sums  : per mesh the exclusive running sum of its tiles' totals
//   k_mesh_scan_add   : C = the tile's offset + the local sum: the mesh's inclusive running sum
//   k_mesh_draw       : one lane per sample: four Philox4x32-10 words -> (uf, u, v); the face is the first f of the mesh
//                       with C[f] > uf * A by a binary search, whose first 12 levels run on every (F / 4096)-th entry of C
//                       staged in LDS and the rest in global memory; the point is (w0 a + w1 b) + w2 c
//   backward          : a gather over the counting-sorted lists of gather_lists.h (query = sample, target = face, one flat
//                       cloud), each list summed in ascending sample order by its own lane (k_mesh_grad_face) or by one
//                       wave (k_mesh_grad_heavy).  No float atomics: two runs give the same bits.
//
// The scan is a chain of roundings of one shape: a thread adds its 8 faces in order, the 256 threads' totals are added in
// thread order, the tiles' totals in tile order, and C[f] = fl(tile offset + fl(thread offset + thread-local sum)).  Every
// step is fl(x + a) with a >= 0 on a fixed x, or the same x carried on, so C never descends and a face of area 0 has
// exactly the C of its predecessor: the search cannot choose it.
#include <math.h>
#include "gather_lists.h"

#pragma clang fp contract(off)

namespace {

constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanBlock * kScanItems;   // faces per workgroup of the scan
constexpr int kDrawBlock = 256;
constexpr int kDrawTable = 4096;     // entries of C a workgroup of the draw stages in LDS (32 KB)
constexpr int kDrawGridCap = 1024;   // workgroups per mesh: a staged table serves many samples
constexpr int kMaxGridY = 65535;
constexpr float kNormalEps = 2.220446e-16f;

// ---- the generator ----------------------------------------------------------------------------------------------
// Philox4x32 with 10 rounds; key = the seed's two halves, counter = (sample lo, sample hi, mesh, 0)
__host__ __device__ inline void mesh_draw_words(uint64_t seed, uint32_t mesh, uint64_t sample, uint32_t (&r)[4]) {
  uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)(sample & 0xffffffffu), c1 = (uint32_t)(sample >> 32), c2 = mesh, c3 = 0u;
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// ---- faces ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ms_load9(const float* __restrict__ src, float (&v)[9]) {
#pragma unroll
  for (int c = 0; c < 9; ++c) v[c] = src[c];
}

// m = (v1 - v0) x (v2 - v0) and |m|; the edges come back for the backward pass
__device__ __forceinline__ float ms_cross(const float (&v)[9], float (&e1)[3], float (&e2)[3], float (&m)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { e1[c] = v[3 + c] - v[c]; e2[c] = v[6 + c] - v[c]; }
  m[0] = e1[1] * e2[2] - e1[2] * e2[1];
  m[1] = e1[2] * e2[0] - e1[0] * e2[2];
  m[2] = e1[0] * e2[1] - e1[1] * e2[0];
  return sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
}

__global__ __launch_bounds__(256) void k_mesh_areas(const float* __restrict__ tris, int64_t n_tris,
                                                    float* __restrict__ areas, float* __restrict__ normals) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tris; t += (int64_t)gridDim.x * blockDim.x) {
    float v[9], e1[3], e2[3], m[3];
    ms_load9(tris + t * 9, v);
    const float len = ms_cross(v, e1, e2, m);
    if (areas) areas[t] = 0.5f * len;
    if (normals) {
      const float d = fmaxf(len, kNormalEps);
#pragma unroll
      for (int c = 0; c < 3; ++c) normals[t * 3 + c] = m[c] / d;
    }
  }
}

// a mesh's rows, kept inside the packed array whatever first / len hold
__device__ __forceinline__ void ms_rows(const int64_t* first, const int64_t* len, int n, int64_t n_tris, int64_t& f0,
                                        int64_t& l) {
  f0 = first[n];
  l = len[n];
  if (f0 < 0 || f0 > n_tris) { f0 = 0; l = 0; }
  if (l < 0) l = 0;
  if (l > n_tris - f0) l = n_tris - f0;
}

// ---- the float64 scan ---------------------------------------------------------------------------------------------
// 64 values, one per lane, added in lane order onto `running` (the same in every lane): returns the lane's exclusive sum
__device__ __forceinline__ double ms_chain64(double x, double& running, int lane) {
  double excl = 0.0;
  for (int i = 0; i < 64; ++i) {
    const double v = __shfl(x, i);
    if (lane == i) excl = running;
    running = running + v;
  }
  return excl;
}

__global__ __launch_bounds__(kScanBlock) void k_mesh_scan_tiles(const float* __restrict__ areas,
                                                                const int64_t* __restrict__ first,
                                                                const int64_t* __restrict__ len, int n_meshes,
                                                                int64_t n_tris, int64_t tiles, double* __restrict__ C,
                                                                double* __restrict__ tile_sums) {
  __shared__ double s_tot[kScanBlock];
  for (int n = blockIdx.y; n < n_meshes; n += gridDim.y) {
    int64_t f0, l;
    ms_rows(first, len, n, n_tris, f0, l);
    for (int64_t tile = blockIdx.x; tile * kScanTile < l; tile += gridDim.x) {   // the same trip count in the whole workgroup
      const int64_t i0 = tile * kScanTile + (int64_t)threadIdx.x * kScanItems;
      double loc[kScanItems];
      double run = 0.0;
#pragma unroll
      for (int k = 0; k < kScanItems; ++k) {
        const float a = (i0 + k < l) ? areas[f0 + i0 + k] : 0.f;
        run = run + (double)a;
        loc[k] = run;
      }
      __syncthreads();                     // the previous tile's readers of s_tot are done
      s_tot[threadIdx.x] = run;
      __syncthreads();
      if (threadIdx.x < 64) {
        double running = 0.0;
#pragma unroll
        for (int c = 0; c < kScanBlock / 64; ++c) {
          const double x = s_tot[c * 64 + threadIdx.x];
          s_tot[c * 64 + threadIdx.x] = ms_chain64(x, running, threadIdx.x);
        }
        if (threadIdx.x == 0) tile_sums[(int64_t)n * tiles + tile] = running;
      }
      __syncthreads();
      const double o = s_tot[threadIdx.x];
#pragma unroll
      for (int k = 0; k < kScanItems; ++k)
        if (i0 + k < l) C[f0 + i0 + k] = o + loc[k];
    }
  }
}

// one wave per mesh: the tiles' totals -> their exclusive running sum, in place
__global__ __launch_bounds__(64) void k_mesh_scan_sums(const int64_t* __restrict__ first, const int64_t* __restrict__ len,
                                                       int n_meshes, int64_t n_tris, int64_t tiles,
                                                       double* __restrict__ tile_sums) {
  const int lane = threadIdx.x;
  for (int n = blockIdx.x; n < n_meshes; n += gridDim.x) {
    int64_t f0, l;
    ms_rows(first, len, n, n_tris, f0, l);
    const int64_t nb = (l + kScanTile - 1) / kScanTile;
    double* ts = tile_sums + (int64_t)n * tiles;
    double running = 0.0;
    for (int64_t b0 = 0; b0 < nb; b0 += 64) {
      const int64_t b = b0 + lane;
      const double x = b < nb ? ts[b] : 0.0;
      const double excl = ms_chain64(x, running, lane);
      if (b < nb) ts[b] = excl;
    }
  }
}

__global__ __launch_bounds__(kScanBlock) void k_mesh_scan_add(const int64_t* __restrict__ first,
                                                              const int64_t* __restrict__ len, int n_meshes,
                                                              int64_t n_tris, int64_t tiles,
                                                              const double* __restrict__ tile_sums,
                                                              double* __restrict__ C) {
  for (int n = blockIdx.y; n < n_meshes; n += gridDim.y) {
    int64_t f0, l;
    ms_rows(first, len, n, n_tris, f0, l);
    // tile 0 starts at 0: nothing to add
    for (int64_t tile = (int64_t)blockIdx.x + 1; tile * kScanTile < l; tile += gridDim.x) {
      const double B = tile_sums[(int64_t)n * tiles + tile];
#pragma unroll
      for (int k = 0; k < kScanItems; ++k) {
        const int64_t i = tile * kScanTile + (int64_t)k * kScanBlock + threadIdx.x;
        if (i < l) C[f0 + i] = B + C[f0 + i];
      }
    }
  }
}

// ---- the draw -------------------------------------------------------------------------------------------------------
struct MsDraw {
  const float* tris;
  const int64_t* first;
  const int64_t* len;
  const double* C;
  float* points;       // (N,S,3)
  float* normals;      // (N,S,3) or null
  int32_t* face_idx;   // (N,S) or null
  float* bary;         // (N,S,3) or null
  int64_t n_tris, n_samples;
  uint64_t seed;
  int n_meshes;
};

__global__ __launch_bounds__(kDrawBlock) void k_mesh_draw(MsDraw a) {
  __shared__ double s_tab[kDrawTable];
  for (int n = blockIdx.y; n < a.n_meshes; n += gridDim.y) {
    int64_t f0, l;
    ms_rows(a.first, a.len, n, a.n_tris, f0, l);
    const double* Cn = a.C + f0;
    const double A = l > 0 ? Cn[l - 1] : 0.0;
    // s_tab[j] = C at the end of the j-th chunk of `stride` faces: the first levels of the search run in LDS
    const int64_t stride = l > kDrawTable ? (l + kDrawTable - 1) / kDrawTable : 1;
    const int chunks = (int)((l + stride - 1) / stride);
    __syncthreads();                       // the previous mesh's readers of s_tab are done
    for (int j = threadIdx.x; j < chunks; j += kDrawBlock) {
      const int64_t e = (j + 1) * stride - 1;
      s_tab[j] = Cn[e < l ? e : l - 1];
    }
    __syncthreads();
    const bool any = l > 0 && A > 0.0 && A <= 1.7976931348623157e308;   // a mesh without area (or with a NaN one): nothing to sample
    for (int64_t s = (int64_t)blockIdx.x * kDrawBlock + threadIdx.x; s < a.n_samples; s += (int64_t)gridDim.x * kDrawBlock) {
      const int64_t row = (int64_t)n * a.n_samples + s;
      float p[3] = {0.f, 0.f, 0.f}, nm[3] = {0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f};
      int32_t face = -1;
      if (any) {
        uint32_t r[4];
        mesh_draw_words(a.seed, (uint32_t)n, (uint64_t)s, r);
        const uint64_t k = ((uint64_t)r[0] << 21) | (uint64_t)(r[1] >> 11);
        const double uf = (double)k * 1.1102230246251565e-16;              // 2^-53: exact
        const float u = (float)(r[2] >> 8) * 5.9604644775390625e-8f;       // 2^-24: exact
        const float v = (float)(r[3] >> 8) * 5.9604644775390625e-8f;
        const double t = uf * A;
        // the first f with C[f] > t; t < A = C[l - 1], so it exists: its chunk first, then inside the chunk
        int cl = 0, ch = chunks - 1;
        while (cl < ch) {
          const int mid = (cl + ch) >> 1;
          if (s_tab[mid] > t) ch = mid;
          else cl = mid + 1;
        }
        int64_t lo = cl * stride, hi = (cl + 1) * stride - 1 < l - 1 ? (cl + 1) * stride - 1 : l - 1;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (Cn[mid] > t) hi = mid;
          else lo = mid + 1;
        }
        face = (int32_t)(f0 + lo);
        const float sq = sqrtf(u);
        w[0] = 1.0f - sq;
        w[1] = sq * (1.0f - v);
        w[2] = sq * v;
        float tv[9];
        ms_load9(a.tris + (f0 + lo) * 9, tv);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = (w[0] * tv[c] + w[1] * tv[3 + c]) + w[2] * tv[6 + c];
        if (a.normals) {
          float e1[3], e2[3], m[3];
          const float d = fmaxf(ms_cross(tv, e1, e2, m), kNormalEps);
#pragma unroll
          for (int c = 0; c < 3; ++c) nm[c] = m[c] / d;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) a.points[row * 3 + c] = p[c];
      if (a.normals) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.normals[row * 3 + c] = nm[c];
      }
      if (a.face_idx) a.face_idx[row] = face;
      if (a.bary) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.bary[row * 3 + c] = w[c];
      }
    }
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// Sample q chose face face_idx[q] with weights bary[q].  d points / d v_k = w_k; the normal is m / max(|m|, eps) of the
// face, so the face's normal gradient is the sum G of its samples' g_normals pushed through that once.
struct MsBack {
  const float* tris;
  const float* bary;
  const float* g_points;    // (Q,3)
  const float* g_normals;   // (Q,3) or null
  float* grad_tris;         // (T,9)
  int64_t n_t;
  GatherView lists;         // one cloud: idx (Q) = the packed face of each sample
  int32_t* heavy;           // (n_t)
  int32_t* heavy_count;
};

// acc[0..8]: sum of w_k g_points per vertex; acc[9..11]: G
__device__ __forceinline__ void ms_add_sample(const MsBack& a, int64_t q, float (&acc)[12]) {
  const float g[3] = {a.g_points[q * 3], a.g_points[q * 3 + 1], a.g_points[q * 3 + 2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float w = a.bary[q * 3 + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[3 * k + c] += w * g[c];
  }
  if (a.g_normals) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[9 + c] += a.g_normals[q * 3 + c];
  }
}

__device__ __forceinline__ void ms_cross3(const float (&x)[3], const float (&y)[3], float (&o)[3]) {
  o[0] = x[1] * y[2] - x[2] * y[1];
  o[1] = x[2] * y[0] - x[0] * y[2];
  o[2] = x[0] * y[1] - x[1] * y[0];
}

// the face's nine gradients from its sums
__device__ __forceinline__ void ms_write_face(const MsBack& a, int64_t f, float (&acc)[12]) {
  if (a.g_normals) {
    float v[9], e1[3], e2[3], m[3], dm[3], de1[3], de2[3];
    ms_load9(a.tris + f * 9, v);
    const float len = ms_cross(v, e1, e2, m);
    const float G[3] = {acc[9], acc[10], acc[11]};
    if (len > kNormalEps) {
      const float nx = m[0] / len, ny = m[1] / len, nz = m[2] / len;
      const float nG = (nx * G[0] + ny * G[1]) + nz * G[2];
      dm[0] = (G[0] - nx * nG) / len;
      dm[1] = (G[1] - ny * nG) / len;
      dm[2] = (G[2] - nz * nG) / len;
    } else {   // the clamped denominator is a constant
#pragma unroll
      for (int c = 0; c < 3; ++c) dm[c] = G[c] / kNormalEps;
    }
    ms_cross3(e2, dm, de1);
    ms_cross3(dm, e1, de2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      acc[c] -= de1[c] + de2[c];
      acc[3 + c] += de1[c];
      acc[6 + c] += de2[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) a.grad_tris[f * 9 + c] = acc[c];
}

// One lane per face: a list of up to kLightList samples is summed here in ascending sample order, a longer one is left
// to k_mesh_grad_heavy, which writes that face.
__global__ __launch_bounds__(256) void k_mesh_grad_face(MsBack a) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < a.n_t; f += (int64_t)gridDim.x * blockDim.x) {
    float acc[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = 0.f;
    const int L = a.lists.cnt[f];
    if (L > kLightList) {
      a.heavy[atomicAdd(a.heavy_count, 1)] = (int32_t)f;   // the order of this list decides nothing: one wave per entry
      continue;
    }
    if (L > 0) {
      gather_lane(gather_list(a.lists, 0, f), L, [&](int q) { ms_add_sample(a, q, acc); });
      ms_write_face(a, f, acc);
    } else {
#pragma unroll
      for (int c = 0; c < 9; ++c) a.grad_tris[f * 9 + c] = 0.f;
    }
  }
}

// One wave per long list (gather_wave): every lane's sum runs in ascending sample order and the 64 sums are added by the
// same butterfly, a fixed order.
__global__ __launch_bounds__(64) void k_mesh_grad_heavy(MsBack a) {
  __shared__ int32_t s_raw[kSortList], s_sorted[kSortList];
  const int lane = threadIdx.x;
  const int count = *a.heavy_count;
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int f = a.heavy[w];
    const int L = a.lists.cnt[f];
    float acc[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = 0.f;
    gather_wave(a.lists, 0, f, L, lane, s_raw, s_sorted, [&](int64_t q) { ms_add_sample(a, q, acc); });
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = iso_wave_sum(acc[c]);
    if (lane == 0) ms_write_face(a, f, acc);
  }
}

inline int64_t ms_tiles(int64_t n_tris) { return n_tris > 0 ? (n_tris + kScanTile - 1) / kScanTile : 1; }

// workspace of iso_mesh_sample: [C: T doubles][tile sums: N * tiles doubles][areas: T floats]
inline int64_t ms_c_bytes(int64_t n_tris) { return iso_align16(8 * n_tris); }
inline int64_t ms_sums_bytes(int n_meshes, int64_t n_tris) { return iso_align16(8 * (int64_t)n_meshes * ms_tiles(n_tris)); }

}  // namespace

extern "C" int iso_mesh_face_areas(const float* tris, int64_t n_tris, float* areas_out, float* normals_out,
                                   void* stream) {
  ISO_REQUIRE(n_tris >= 0, ISO_ERR_INVALID, "iso_mesh_face_areas: bad sizes");
  ISO_REQUIRE(n_tris <= 0x7fffffff, ISO_ERR_UNSUPPORTED, "iso_mesh_face_areas: 32-bit face indices");
  if (n_tris == 0 || (!areas_out && !normals_out)) return ISO_OK;
  ISO_REQUIRE(tris, ISO_ERR_INVALID, "iso_mesh_face_areas: null pointer");
  hipLaunchKernelGGL(k_mesh_areas, dim3(iso_stream_grid(n_tris, 256)), dim3(256), 0, (hipStream_t)stream, tris, n_tris,
                     areas_out, normals_out);
  ISO_CHECK_LAUNCH("iso_mesh_face_areas");
  return ISO_OK;
}

extern "C" int64_t iso_mesh_sample_workspace_bytes(int n_meshes, int64_t n_tris) {
  if (n_meshes < 0) n_meshes = 0;
  if (n_tris < 0) n_tris = 0;
  return ms_c_bytes(n_tris) + ms_sums_bytes(n_meshes, n_tris) + iso_align16(4 * n_tris) + 16;
}

extern "C" int iso_mesh_sample(const float* tris, const int64_t* tris_first, const int64_t* tris_len, int n_meshes,
                               int64_t n_tris, int64_t n_samples, int64_t seed, float* points_out, float* normals_out,
                               int32_t* face_idx_out, float* bary_out, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  ISO_REQUIRE(n_meshes >= 0 && n_tris >= 0 && n_samples >= 0, ISO_ERR_INVALID, "iso_mesh_sample: bad sizes");
  ISO_REQUIRE(n_tris <= 0x7fffffff, ISO_ERR_UNSUPPORTED, "iso_mesh_sample: 32-bit face indices");
  ISO_REQUIRE(n_samples <= 0x7fffffff && (int64_t)n_meshes * n_samples <= 0x7fffffff, ISO_ERR_UNSUPPORTED,
              "iso_mesh_sample: 32-bit sample rows (N * S < 2^31)");
  if (n_meshes == 0 || n_samples == 0) return ISO_OK;
  ISO_REQUIRE(points_out && tris_first && tris_len && (tris || n_tris == 0), ISO_ERR_INVALID,
              "iso_mesh_sample: null pointer");
  ISO_REQUIRE(workspace && workspace_bytes >= iso_mesh_sample_workspace_bytes(n_meshes, n_tris), ISO_ERR_WORKSPACE,
              "iso_mesh_sample: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "iso_mesh_sample: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  double* C = reinterpret_cast<double*>(workspace);
  double* tile_sums = reinterpret_cast<double*>((char*)workspace + ms_c_bytes(n_tris));
  float* areas = reinterpret_cast<float*>((char*)workspace + ms_c_bytes(n_tris) + ms_sums_bytes(n_meshes, n_tris));
  const int64_t tiles = ms_tiles(n_tris);
  const int gy = n_meshes < kMaxGridY ? n_meshes : kMaxGridY;
  if (n_tris > 0) {
    const int gt = (int)(tiles < 65536 ? tiles : 65536);
    hipLaunchKernelGGL(k_mesh_areas, dim3(iso_stream_grid(n_tris, 256)), dim3(256), 0, s, tris, n_tris, areas,
                       (float*)nullptr);
    hipLaunchKernelGGL(k_mesh_scan_tiles, dim3(gt, gy), dim3(kScanBlock), 0, s, areas, tris_first, tris_len, n_meshes,
                       n_tris, tiles, C, tile_sums);
    hipLaunchKernelGGL(k_mesh_scan_sums, dim3(gy), dim3(64), 0, s, tris_first, tris_len, n_meshes, n_tris, tiles,
                       tile_sums);
    if (tiles > 1)
      hipLaunchKernelGGL(k_mesh_scan_add, dim3(gt, gy), dim3(kScanBlock), 0, s, tris_first, tris_len, n_meshes, n_tris,
                         tiles, tile_sums, C);
  }
  MsDraw a{tris, tris_first, tris_len, C, points_out, normals_out, face_idx_out, bary_out, n_tris, n_samples,
           (uint64_t)seed, n_meshes};
  hipLaunchKernelGGL(k_mesh_draw, dim3(iso_capped_grid(n_samples, kDrawBlock, kDrawGridCap), gy), dim3(kDrawBlock), 0, s, a);
  ISO_CHECK_LAUNCH("iso_mesh_sample");
  return ISO_OK;
}

// workspace of iso_mesh_sample_backward: gather_lists.h's, with n_tris target rows and n_rows query rows
extern "C" int64_t iso_mesh_sample_backward_workspace_bytes(int64_t n_tris, int64_t n_rows) {
  if (n_tris < 0) n_tris = 0;
  if (n_rows < 0) n_rows = 0;
  return gather_workspace_bytes(n_tris, n_rows, n_tris, 1);
}

extern "C" int iso_mesh_sample_backward(const float* tris, const int32_t* face_idx, const float* bary,
                                        const float* g_points, const float* g_normals, float* grad_tris,
                                        int64_t n_tris, int64_t n_rows, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  ISO_REQUIRE(n_tris >= 0 && n_rows >= 0, ISO_ERR_INVALID, "iso_mesh_sample_backward: bad sizes");
  ISO_REQUIRE(n_tris <= 0x7fffffff && n_rows <= 0x7fffffff, ISO_ERR_UNSUPPORTED,
              "iso_mesh_sample_backward: 32-bit indices");
  if (n_tris == 0 || !grad_tris) return ISO_OK;
  ISO_REQUIRE(tris, ISO_ERR_INVALID, "iso_mesh_sample_backward: null pointer");
  ISO_REQUIRE(n_rows == 0 || (face_idx && bary && g_points), ISO_ERR_INVALID, "iso_mesh_sample_backward: null pointer");
  ISO_REQUIRE(workspace && workspace_bytes >= iso_mesh_sample_backward_workspace_bytes(n_tris, n_rows), ISO_ERR_WORKSPACE,
              "iso_mesh_sample_backward: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID,
              "iso_mesh_sample_backward: workspace must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  const GatherWorkspace w = gather_carve(workspace, n_tris, n_rows);
  const GatherView lists{face_idx, w.cnt, w.off, w.slot, w.list, n_rows, n_tris, n_rows, n_tris};
  const int rc = gather_build(GatherViews{{lists, lists}}, 1, 1, n_rows, w, n_tris, n_tris, 1, s);
  if (rc != ISO_OK) return rc;
  MsBack a{tris, bary, g_points, g_normals, grad_tris, n_tris, lists, w.heavy, w.heavy_count};
  hipLaunchKernelGGL(k_mesh_grad_face, dim3(iso_capped_grid(n_tris, 256, 4096)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_mesh_grad_heavy, dim3((int)(n_tris < 2048 ? n_tris : 2048)), dim3(64), 0, s, a);
  ISO_CHECK_LAUNCH("iso_mesh_sample_backward");
  return ISO_OK;
}

extern "C" int iso_mesh_sample_draw(int64_t seed, int mesh, int64_t sample, uint32_t* out_words) {
  ISO_REQUIRE(out_words, ISO_ERR_INVALID, "iso_mesh_sample_draw: null pointer");
  uint32_t r[4];
  mesh_draw_words((uint64_t)seed, (uint32_t)mesh, (uint64_t)sample, r);
  for (int i = 0; i < 4; ++i) out_words[i] = r[i];
  return ISO_OK;
}
