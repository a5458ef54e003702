// The zero level set of a sampled SDF as an indexed triangle mesh for gfx950: marching tetrahedra on the Kuhn split of
// every grid cell (include/isopoints.h section N has the rule, DESIGN.md 3.4j the reasons).  It stands where the reference
// copies the volume to the host for skimage.measure.marching_cubes_lewiner (DSS/utils/__init__.py:569-655).
//
// Every vertex sits on a mesh edge -- an axis edge, a face diagonal or the body diagonal that STARTS at a grid point, 7
// slots per point -- so a vertex has one owner and an index that is a scan: no hashing, no welding pass, no atomics, the
// same bits on every run.  Two passes around one exclusive scan (iso_prefix_sum over both count rows at once):
//   k_mt_classify  one 4 x 4 x 64 tile of points per 256-lane workgroup, staged with a one-point halo through LDS
//                  (5 x 5 x 65 floats): a lane walks the tile's 4 points along i at its (j, k) and keeps the 4 inside bits
//                  of the plane it shares with the next point.  Per point: the 7-bit mask of active slots, the vertex
//                  count and the cell's triangle count; a cell whose 8 corners agree leaves after one compare.
//   k_mt_emit      reads the masks four points to a 32-bit load; the few points with an active slot interpolate their
//                  vertices and, where they start a cell, write its triangles.  A triangle corner is a (owner point, slot)
//                  pair: two loads (the owner's mask and vertex offset) and a popcount give its index.
// The 16 cases of a tetrahedron are not typed in: tri_code() derives them at compile time from the inside mask and the
// tetrahedron's orientation (the sign of the axis permutation).  The tables, the inside test and the vertex on a slot are
// in mesh_tables.h, which the block-sparse kernels (mesh_extract_sparse.hip) share.
#include "mesh_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int TI = 4, TJ = 4, TK = 64;                    // points of a tile; lane = (tj, tk), walks i
constexpr int HI = TI + 1, HJ = TJ + 1, HK = TK + 1;      // with the halo: the far corners of the last cells
constexpr int MT_BLOCK = 256;
constexpr int MT_MAX_N = 1024;

// inside bits of the four points (j, k), (j+1, k), (j, k+1), (j+1, k+1) of one i-plane of the staged tile
__device__ __forceinline__ unsigned plane_bits(const float* col, float iso) {
  return mt_inside(col[0], iso) | (mt_inside(col[HK], iso) << 1) | (mt_inside(col[1], iso) << 2) | (mt_inside(col[HK + 1], iso) << 3);
}
// corner mask of a cell from the plane bits of its near (x) and far (x + 1) side
__device__ __forceinline__ unsigned corner_mask(unsigned lo, unsigned hi) {
  return (lo & 1u) | ((hi & 1u) << 1) | (((lo >> 1) & 1u) << 2) | (((lo >> 2) & 1u) << 3) | (((hi >> 1) & 1u) << 4) |
         (((hi >> 2) & 1u) << 5) | (((lo >> 3) & 1u) << 6) | (((hi >> 3) & 1u) << 7);
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------
// amask[p]: the active slots of point p; cnt[p]: their number; cnt[n_points + p]: the triangles of the cell that starts at p
// (0 where none starts); partial[2 b], [2 b + 1]: the two sums over workgroup b's tile.
__global__ __launch_bounds__(MT_BLOCK) void k_mt_classify(const float* __restrict__ values, int nx, int ny, int nz, float iso,
                                                          uint8_t* __restrict__ amask, int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ partial) {
  __shared__ float tile[HI * HJ * HK];
  __shared__ int red[MT_BLOCK / 64];
  const int i0 = blockIdx.z * TI, j0 = blockIdx.y * TJ, k0 = blockIdx.x * TK;
  for (int e = threadIdx.x; e < HI * HJ * HK; e += MT_BLOCK) {
    const int lk = e % HK, r = e / HK, lj = r % HJ, li = r / HJ;
    const int gi = i0 + li, gj = j0 + lj, gk = k0 + lk;
    tile[e] = (gi < nx && gj < ny && gk < nz) ? values[((int64_t)gi * ny + gj) * nz + gk] : 0.f;   // never looked at
  }
  __syncthreads();
  const int tk = threadIdx.x & 63, tj = threadIdx.x >> 6;
  const int gj = j0 + tj, gk = k0 + tk;
  const int64_t n_points = (int64_t)nx * ny * nz;
  int nv = 0, nt = 0;
  if (gj < ny && gk < nz) {
    const bool ey = gj + 1 < ny, ez = gk + 1 < nz;
    const float* col = tile + tj * HK + tk;
    unsigned lo = plane_bits(col, iso);
#pragma unroll
    for (int li = 0; li < TI; ++li) {
      const int gi = i0 + li;
      const unsigned hi = plane_bits(col + (li + 1) * HJ * HK, iso);
      if (gi < nx) {
        const unsigned em = exist_mask(gi + 1 < nx, ey, ez);
        const unsigned own = lo & 1u;
        // a corner outside the grid takes the point's own side: its slot is never active
        const unsigned cm = (corner_mask(lo, hi) & em) | (own ? (~em & 0xffu) : 0u);
        int v = 0, t = 0;
        unsigned am = 0;
        if (cm != 0u && cm != 0xffu) {
          am = ((cm >> 1) ^ (own ? 0x7fu : 0u)) & 0x7fu;
          v = __popc(am);
          t = em == 0xffu ? cell_tris(cm) : 0;
        }
        const int64_t p = ((int64_t)gi * ny + gj) * nz + gk;
        amask[p] = (uint8_t)am;
        cnt[p] = v;
        cnt[n_points + p] = t;
        nv += v;
        nt += t;
      }
      lo = hi;
    }
  }
  int tv, tt;
  iso_block_excl_scan<MT_BLOCK / 64>(nv, tv, red);
  iso_block_excl_scan<MT_BLOCK / 64>(nt, tt, red);
  if (threadIdx.x == 0) {
    const int64_t b = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[2 * b] = tv;
    partial[2 * b + 1] = tt;
  }
}

// totals[0] = vertices, totals[1] = faces: the 64-bit sums of the tiles' 32-bit sums, in a fixed order
__global__ __launch_bounds__(1024) void k_mt_totals(const int32_t* __restrict__ partial, int64_t n_blocks, int64_t* __restrict__ totals) {
  __shared__ long long red[2][1024];
  long long sv = 0, st = 0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += 1024) {
    sv += partial[2 * b];
    st += partial[2 * b + 1];
  }
  red[0][threadIdx.x] = sv;
  red[1][threadIdx.x] = st;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[0] = red[0][0];
    totals[1] = red[1][0];
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------
// the triangles of tetrahedron T of the cell that starts at point p
template <int T>
__device__ __forceinline__ void emit_tet(unsigned cm, int p, int sI, int sJ, const uint8_t* __restrict__ amask,
                                         const int32_t* __restrict__ voff, int32_t* __restrict__ faces, int64_t face_cap,
                                         int64_t& f) {
  constexpr uint32_t owner = tet_owner_pack(T), slot = tet_slot_pack(T);
  const uint32_t code = kTri.v[tet_odd(T) ? 1 : 0][tet_mask<T>(cm)];
  const int n = (int)(code & 3u);
  for (int q = 0; q < n; ++q) {
    int32_t idx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned e = (code >> (2 + 3 * (3 * q + c))) & 7u;
      const unsigned oc = (owner >> (3 * e)) & 7u, sl = (slot >> (3 * e)) & 7u;
      const int o = p + ((oc & 1u) ? sI : 0) + ((oc & 2u) ? sJ : 0) + (int)(oc >> 2);
      idx[c] = voff[o] + __popc((unsigned)amask[o] & ((1u << sl) - 1u));
    }
    if (f < face_cap) {
      faces[3 * f] = idx[0];
      faces[3 * f + 1] = idx[1];
      faces[3 * f + 2] = idx[2];
    }
    ++f;
  }
}

__device__ __forceinline__ void emit_point(const float* __restrict__ values, const MtGrid& g, int p, unsigned am,
                                           const uint8_t* __restrict__ amask, const int32_t* __restrict__ voff,
                                           const int32_t* __restrict__ toff, float* __restrict__ verts, int64_t vert_cap,
                                           int32_t* __restrict__ faces, int64_t face_cap) {
  const int k = p % g.nz, r = p / g.nz, j = r % g.ny, i = r / g.ny;
  const int sJ = g.nz, sI = g.ny * g.nz;
  const bool ex = i + 1 < g.nx, ey = j + 1 < g.ny, ez = k + 1 < g.nz;
  const unsigned em = exist_mask(ex, ey, ez);
  float v[8];
  v[0] = values[p];
#pragma unroll
  for (int c = 1; c < 8; ++c) {
    const int code = kSlotCode[c - 1];
    v[c] = ((em >> c) & 1u) ? values[p + ((code & 1) ? sI : 0) + ((code & 2) ? sJ : 0) + (code >> 2)] : v[0];
  }
  int64_t vi = voff[p];
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    if ((am >> s) & 1u) {
      float pos[3];
      mt_vertex(g, i, j, k, kSlotCode[s], v[0], v[s + 1], pos);
      if (vi < vert_cap) {
#pragma unroll
        for (int d = 0; d < 3; ++d) verts[3 * vi + d] = pos[d];
      }
      ++vi;
    }
  }
  if (em == 0xffu) {
    unsigned cm = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) cm |= mt_inside(v[c], g.iso) << c;
    int64_t f = toff[p];
    emit_tet<0>(cm, p, sI, sJ, amask, voff, faces, face_cap, f);
    emit_tet<1>(cm, p, sI, sJ, amask, voff, faces, face_cap, f);
    emit_tet<2>(cm, p, sI, sJ, amask, voff, faces, face_cap, f);
    emit_tet<3>(cm, p, sI, sJ, amask, voff, faces, face_cap, f);
    emit_tet<4>(cm, p, sI, sJ, amask, voff, faces, face_cap, f);
    emit_tet<5>(cm, p, sI, sJ, amask, voff, faces, face_cap, f);
  }
}

// amask is 16-byte aligned and padded to a multiple of 4 bytes: four points to a load
__global__ __launch_bounds__(MT_BLOCK) void k_mt_emit(const float* __restrict__ values, MtGrid g,
                                                      const uint8_t* __restrict__ amask, const int32_t* __restrict__ voff,
                                                      const int32_t* __restrict__ toff, float* __restrict__ verts,
                                                      int64_t vert_cap, int32_t* __restrict__ faces, int64_t face_cap) {
  const int64_t n_points = (int64_t)g.nx * g.ny * g.nz, n_words = (n_points + 3) / 4;
  for (int64_t w = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * MT_BLOCK) {
    const uint32_t four = reinterpret_cast<const uint32_t*>(amask)[w];
    if (four == 0u) continue;
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
      const unsigned am = (four >> (8 * b)) & 0xffu;
      const int64_t p = 4 * w + b;
      if (am != 0u && p < n_points) emit_point(values, g, (int)p, am, amask, voff, toff, verts, vert_cap, faces, face_cap);
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct MtLayout {
  int64_t n_points, n_blocks;
  int gx, gy, gz;
  int64_t cnt, off, amask, partial, scan, scan_bytes, bytes;      // byte offsets into the workspace
};

MtLayout mt_layout(int nx, int ny, int nz) {
  MtLayout L;
  L.n_points = (int64_t)nx * ny * nz;
  L.gx = iso_div_up(nz, TK);
  L.gy = iso_div_up(ny, TJ);
  L.gz = iso_div_up(nx, TI);
  L.n_blocks = (int64_t)L.gx * L.gy * L.gz;
  L.cnt = 0;
  L.off = L.cnt + iso_align16(8 * L.n_points);
  L.amask = L.off + iso_align16(8 * L.n_points);
  L.partial = L.amask + iso_align16(L.n_points);
  L.scan = L.partial + iso_align16(8 * L.n_blocks);
  L.scan_bytes = iso_prefix_sum_workspace_bytes(L.n_points, 2);
  L.bytes = L.scan + iso_align16(L.scan_bytes);
  return L;
}

int mt_check_grid(const char* fn, int nx, int ny, int nz, float iso) {
  ISO_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, ISO_ERR_INVALID, "%s: a volume needs at least 2 points per axis, got %d x %d x %d",
              fn, nx, ny, nz);
  ISO_REQUIRE(nx <= MT_MAX_N && ny <= MT_MAX_N && nz <= MT_MAX_N, ISO_ERR_UNSUPPORTED,
              "%s: at most %d points per axis, got %d x %d x %d", fn, MT_MAX_N, nx, ny, nz);
  ISO_REQUIRE(fabsf(iso) <= FLT_MAX, ISO_ERR_INVALID, "%s: the level must be finite", fn);
  return ISO_OK;
}

}  // namespace

extern "C" int64_t iso_meshextract_workspace_bytes(int nx, int ny, int nz) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > MT_MAX_N || ny > MT_MAX_N || nz > MT_MAX_N) return 0;
  return mt_layout(nx, ny, nz).bytes;
}

extern "C" int iso_meshextract_count(const float* values, int nx, int ny, int nz, float iso, int64_t* totals,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "iso_meshextract_count";
  const int rc = mt_check_grid(fn, nx, ny, nz, iso);
  if (rc != ISO_OK) return rc;
  ISO_REQUIRE(values && totals && workspace, ISO_ERR_INVALID, "%s: null pointer", fn);
  const MtLayout L = mt_layout(nx, ny, nz);
  ISO_REQUIRE(workspace_bytes >= L.bytes, ISO_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld)", fn,
              (long long)workspace_bytes, (long long)L.bytes);
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "%s: the workspace must be 16-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int32_t* partial = (int32_t*)(ws + L.partial);
  hipLaunchKernelGGL(k_mt_classify, dim3(L.gx, L.gy, L.gz), dim3(MT_BLOCK), 0, s, values, nx, ny, nz, iso,
                     (uint8_t*)(ws + L.amask), cnt, partial);
  hipLaunchKernelGGL(k_mt_totals, dim3(1), dim3(1024), 0, s, partial, L.n_blocks, totals);
  ISO_CHECK_LAUNCH(fn);
  return iso_prefix_sum(cnt, (int32_t*)(ws + L.off), L.n_points, 2, L.n_points, ws + L.scan, L.scan_bytes, stream);
}

extern "C" int iso_meshextract_emit(const float* values, int nx, int ny, int nz, float ox, float oy, float oz, float sx,
                                     float sy, float sz, float iso, const int64_t* totals, float* verts, int64_t vert_capacity,
                                     int32_t* faces, int64_t face_capacity, const void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  const char* fn = "iso_meshextract_emit";
  const int rc = mt_check_grid(fn, nx, ny, nz, iso);
  if (rc != ISO_OK) return rc;
  ISO_REQUIRE(fabsf(ox) <= FLT_MAX && fabsf(oy) <= FLT_MAX && fabsf(oz) <= FLT_MAX, ISO_ERR_INVALID, "%s: the origin must be finite", fn);
  ISO_REQUIRE(sx > 0.f && sy > 0.f && sz > 0.f && sx <= FLT_MAX && sy <= FLT_MAX && sz <= FLT_MAX, ISO_ERR_INVALID,
              "%s: the spacing must be positive and finite", fn);
  ISO_REQUIRE(values && totals && workspace, ISO_ERR_INVALID, "%s: null pointer", fn);
  ISO_REQUIRE(vert_capacity >= 0 && face_capacity >= 0, ISO_ERR_INVALID, "%s: negative capacity", fn);
  const MtLayout L = mt_layout(nx, ny, nz);
  ISO_REQUIRE(workspace_bytes >= L.bytes, ISO_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld)", fn,
              (long long)workspace_bytes, (long long)L.bytes);
  hipStream_t s = (hipStream_t)stream;
  // the one host read of the entry: the counted totals, to refuse outputs that cannot hold them
  int64_t tot[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(tot, totals, sizeof(tot), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  ISO_REQUIRE(e == hipSuccess, ISO_ERR_LAUNCH, "%s: reading the totals failed: %s", fn, hipGetErrorString(e));
  ISO_REQUIRE(tot[0] < (1ll << 31) && tot[1] < (1ll << 31), ISO_ERR_UNSUPPORTED,
              "%s: %lld vertices, %lld faces; the limit is 2^31 - 1 of each", fn, (long long)tot[0], (long long)tot[1]);
  ISO_REQUIRE(vert_capacity >= tot[0] && face_capacity >= tot[1], ISO_ERR_INVALID,
              "%s: room for %lld vertices and %lld faces, counted %lld and %lld", fn, (long long)vert_capacity,
              (long long)face_capacity, (long long)tot[0], (long long)tot[1]);
  if (tot[0] == 0 && tot[1] == 0) return ISO_OK;
  ISO_REQUIRE(verts && (faces || tot[1] == 0), ISO_ERR_INVALID, "%s: null output", fn);
  const char* ws = (const char*)workspace;
  const int32_t* off = (const int32_t*)(ws + L.off);
  MtGrid g = {nx, ny, nz, {ox, oy, oz}, {sx, sy, sz}, iso};
  hipLaunchKernelGGL(k_mt_emit, dim3(iso_stream_grid((L.n_points + 3) / 4, MT_BLOCK)), dim3(MT_BLOCK), 0, s, values, g,
                     (const uint8_t*)(ws + L.amask), off, off + L.n_points, verts, vert_capacity, faces, face_capacity);
  ISO_CHECK_LAUNCH(fn);
  return ISO_OK;
}
