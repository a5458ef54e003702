// Block-sparse marching tetrahedra for gfx950: the rule of mesh_extract.hip (mesh_tables.h holds it for both) over a list of
// 8 x 8 x 8 bricks of grid points instead of the whole box (include/isopoints.h section O).  Work and memory
// follow the surface's area, sides go up to 4096, and where the bricks cover the surface the mesh is the dense one bit for bit.
//
// Every grid point is stored once: brick b holds the points 8 b .. 8 b + 7 per axis, no halo.  A cell whose base lies in
// brick b (cell-block b) reaches into the bricks b + {0,1}^3; they are found through a table with one int32 per brick of
// the grid (-1 = not in the list).  Vertices are numbered by (brick in list order, local point, slot), faces by (brick, local
// cell, tetrahedron, triangle): one exclusive scan over S * 512 counts, no atomics on global memory, the same bits every run.
//   k_mts_table     list slot of every listed brick into the table
//   k_mts_classify  one workgroup per listed brick: the 9 x 9 x 9 values its cells touch gathered into LDS (rows of 8 floats
//                   from up to 8 bricks), then per point the mask of live and active slots, the vertex count, the cell's
//                   triangle count, and per brick the need byte and the two sums.  A brick whose 729 inside flags agree
//                   writes zeros and leaves.
//   k_mts_totals    the 64-bit totals: vertices, faces, set need bits, coords outside the grid
//   k_mts_emit      one workgroup per brick with a vertex: a lane with an active slot gathers its 8 corner values through
//                   the table, writes its vertices and, in a cell-active brick, its cell's triangles; a triangle corner is
//                   (owner point, slot): the owner's brick through the table, its mask and offset, a popcount.
#include "mesh_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int MTS_BLOCK = 512;                            // one lane per point of a brick: local index (i * 8 + j) * 8 + k
constexpr int MTS_ST = 9;                                 // staged points per axis: the brick and the far corners of its cells
constexpr int MTS_STAGED = MTS_ST * MTS_ST * MTS_ST;
constexpr int MTS_MAX_N = 4096;

struct MtsDims {
  int nx, ny, nz, bx, by, bz;                             // grid points and bricks per axis
};

MtsDims mts_dims(int nx, int ny, int nz) { return {nx, ny, nz, (nx + 7) / 8, (ny + 7) / 8, (nz + 7) / 8}; }

__device__ __forceinline__ bool mts_brick_in_grid(const MtsDims& d, int bi, int bj, int bk) {
  return bi >= 0 && bj >= 0 && bk >= 0 && bi < d.bx && bj < d.by && bk < d.bz;
}
__device__ __forceinline__ int64_t mts_brick_lin(const MtsDims& d, int bi, int bj, int bk) { return ((int64_t)bi * d.by + bj) * d.bz + bk; }

// the cell offsets d (bit d of the result) whose cell with base p - d contains slot s of p: d & code(s) == 0
constexpr unsigned cells_of_slot(int s) {
  unsigned m = 0;
  for (int d = 0; d < 8; ++d)
    if ((d & kSlotCode[s]) == 0) m |= 1u << d;
  return m;
}
// the slots s (bit s) of p that the cell with base p - d contains
constexpr unsigned slots_of_cell(int d) {
  unsigned m = 0;
  for (int s = 0; s < 7; ++s)
    if ((d & kSlotCode[s]) == 0) m |= 1u << s;
  return m;
}

__global__ void k_mts_fill(int32_t* __restrict__ p, int64_t n, int32_t v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void k_mts_table(const int32_t* __restrict__ coords, int64_t S, MtsDims d, int32_t* __restrict__ table) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int bi = coords[3 * s], bj = coords[3 * s + 1], bk = coords[3 * s + 2];
  if (mts_brick_in_grid(d, bi, bj, bk)) table[mts_brick_lin(d, bi, bj, bk)] = (int32_t)s;
}

// nb[o]: the list slot of brick b + o (-1: outside the grid or not listed); nb[0] is the brick itself.  Lanes 0..7.
__device__ __forceinline__ void mts_neighbours(const MtsDims& d, const int32_t* __restrict__ table, int s, int bi, int bj, int bk,
                                               int* nb) {
  const int o = threadIdx.x;
  if (o < 8) {
    const int ni = bi + (o & 1), nj = bj + ((o >> 1) & 1), nk = bk + (o >> 2);
    nb[o] = o == 0 ? s : (mts_brick_in_grid(d, ni, nj, nk) ? table[mts_brick_lin(d, ni, nj, nk)] : -1);
  }
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------
// Row r = s * 512 + local point.  amask[r]: the live slots of the point whose ends differ; cnt[r]: their number;
// cnt[n_rows + r]: the triangles of the cell that starts at the point (0 unless the brick is cell-active and the cell exists);
// partial[2 s], [2 s + 1]: the brick's two sums; need[s]: section O's need byte.
__global__ __launch_bounds__(MTS_BLOCK) void k_mts_classify(const float* __restrict__ values, const int32_t* __restrict__ coords,
                                                            const uint8_t* __restrict__ cell_active, int64_t S, MtsDims d, float iso,
                                                            const int32_t* __restrict__ table, uint8_t* __restrict__ amask,
                                                            int32_t* __restrict__ cnt, int32_t* __restrict__ partial,
                                                            uint8_t* __restrict__ need) {
  __shared__ float tile[MTS_STAGED];
  __shared__ int nb[8];
  __shared__ int red[MTS_BLOCK / 64];
  __shared__ unsigned lower_active, need_bits;
  const int s = blockIdx.x, t = threadIdx.x;
  const int64_t n_rows = S * MTS_BLOCK, row = (int64_t)s * MTS_BLOCK + t;
  const int bi = coords[3 * s], bj = coords[3 * s + 1], bk = coords[3 * s + 2];
  bool quiet = !mts_brick_in_grid(d, bi, bj, bk);           // a brick outside the grid counts nothing (k_mts_totals reports it)
  if (!quiet) {
    mts_neighbours(d, table, s, bi, bj, bk, nb);
    if (t < 64) {                                           // bit o: cell-block b - o exists and is cell-active
      bool act = false;
      if (t < 8) {
        const int li = bi - (t & 1), lj = bj - ((t >> 1) & 1), lk = bk - (t >> 2);
        const int slot = t == 0 ? s : (mts_brick_in_grid(d, li, lj, lk) ? table[mts_brick_lin(d, li, lj, lk)] : -1);
        act = slot >= 0 && cell_active[slot] != 0;
      }
      const unsigned long long bal = __ballot(act);
      if (t == 0) {
        lower_active = (unsigned)bal & 0xffu;
        need_bits = 0u;
      }
    }
    __syncthreads();
    // the 9 x 9 x 9 points of the brick's cells: rows of 8 floats from the brick and its 7 upper neighbours.  A point outside
    // the grid or in a brick that is not listed takes the brick's first value: never looked at where a slot is live, and it
    // cannot break the agreement of the inside flags
    const float first = values[(int64_t)s * MTS_BLOCK];
    int n_inside = 0;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int e = t + round * MTS_BLOCK;
      bool in = false;
      if (e < MTS_STAGED) {
        const int lk = e % MTS_ST, r = e / MTS_ST, lj = r % MTS_ST, li = r / MTS_ST;
        const int slot = nb[(li >> 3) | ((lj >> 3) << 1) | ((lk >> 3) << 2)];
        const bool there = slot >= 0 && 8 * bi + li < d.nx && 8 * bj + lj < d.ny && 8 * bk + lk < d.nz;
        const float v = there ? values[(int64_t)slot * MTS_BLOCK + (((li & 7) * 8 + (lj & 7)) * 8 + (lk & 7))] : first;
        tile[e] = v;
        in = mt_inside(v, iso) != 0u;
      }
      n_inside += __syncthreads_count(in);
    }
    quiet = n_inside == 0 || n_inside == MTS_STAGED;
  }
  if (quiet) {                                              // uniform over the workgroup
    amask[row] = 0;
    cnt[row] = 0;
    cnt[n_rows + row] = 0;
    if (t == 0) {
      partial[2 * s] = 0;
      partial[2 * s + 1] = 0;
      need[s] = 0;
    }
    return;
  }
  const int li = t >> 6, lj = (t >> 3) & 7, lk = t & 7;
  const int gi = 8 * bi + li, gj = 8 * bj + lj, gk = 8 * bk + lk;
  int nv = 0, nt = 0;
  unsigned am = 0, nd = 0;
  if (gi < d.nx && gj < d.ny && gk < d.nz) {
    const bool ex = gi + 1 < d.nx, ey = gj + 1 < d.ny, ez = gk + 1 < d.nz;
    const unsigned zl = (li == 0 ? 1u : 0u) | (lj == 0 ? 2u : 0u) | (lk == 0 ? 4u : 0u);   // axes on which p - 1 is in a lower brick
    const unsigned ca = lower_active;
    unsigned cell_there = 0, cell_marched = 0;              // bit dd: the cell with base p - dd exists / is in a cell-active block
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) {
      const bool there = ((dd & 1) ? gi >= 1 : ex) && ((dd & 2) ? gj >= 1 : ey) && ((dd & 4) ? gk >= 1 : ez);
      cell_there |= there ? 1u << dd : 0u;
      cell_marched |= (there && ((ca >> (dd & zl)) & 1u)) ? 1u << dd : 0u;
    }
    unsigned live = 0, cm = 0;
#pragma unroll
    for (int sl = 0; sl < 7; ++sl) live |= (cell_marched & cells_of_slot(sl)) ? 1u << sl : 0u;
    const float* at = tile + (li * MTS_ST + lj) * MTS_ST + lk;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int code = c == 0 ? 0 : kSlotCode[c - 1];
      cm |= mt_inside(at[((code & 1) * MTS_ST + ((code >> 1) & 1)) * MTS_ST + (code >> 2)], iso) << c;
    }
    const unsigned own = cm & 1u;
    am = ((cm >> 1) ^ (own ? 0x7fu : 0u)) & live;
    nv = __popc(am);
    if ((ca & 1u) && exist_mask(ex, ey, ez) == 0xffu) nt = cell_tris(cm);
    if (am != 0u) {
#pragma unroll
      for (int dd = 0; dd < 8; ++dd)
        if (((cell_there & ~cell_marched) >> dd) & 1u)
          if (am & slots_of_cell(dd)) nd |= 1u << (dd & zl);
    }
  }
  amask[row] = (uint8_t)am;
  cnt[row] = nv;
  cnt[n_rows + row] = nt;
  if (nd != 0u) atomicOr(&need_bits, nd);                   // LDS, and an OR: the order does not show
  int tv, tt;
  iso_block_excl_scan<MTS_BLOCK / 64>(nv, tv, red);
  iso_block_excl_scan<MTS_BLOCK / 64>(nt, tt, red);
  if (t == 0) {
    partial[2 * s] = tv;
    partial[2 * s + 1] = tt;
    need[s] = (uint8_t)need_bits;
  }
}

// totals[0] = vertices, [1] = faces, [2] = set need bits, [3] = bricks whose coords are outside the grid: 64-bit sums in a
// fixed order
__global__ __launch_bounds__(1024) void k_mts_totals(const int32_t* __restrict__ partial, const uint8_t* __restrict__ need,
                                                     const int32_t* __restrict__ coords, int64_t S, MtsDims d,
                                                     int64_t* __restrict__ totals) {
  __shared__ long long red[4][1024];
  long long acc[4] = {0, 0, 0, 0};
  for (int64_t s = threadIdx.x; s < S; s += 1024) {
    acc[0] += partial[2 * s];
    acc[1] += partial[2 * s + 1];
    acc[2] += __popc((unsigned)need[s]);
    acc[3] += mts_brick_in_grid(d, coords[3 * s], coords[3 * s + 1], coords[3 * s + 2]) ? 0 : 1;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) totals[threadIdx.x] = red[threadIdx.x][0];
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------
// the row of the point at local (li, lj, lk) + offset code, li .. in 0..8: through nb to the brick that stores it; -1 if that
// brick is not listed
__device__ __forceinline__ int64_t mts_row(const int* nb, int li, int lj, int lk) {
  const int slot = nb[(li >> 3) | ((lj >> 3) << 1) | ((lk >> 3) << 2)];
  return slot < 0 ? -1 : (int64_t)slot * MTS_BLOCK + (((li & 7) * 8 + (lj & 7)) * 8 + (lk & 7));
}

template <int T>
__device__ __forceinline__ void mts_emit_tet(unsigned cm, const int* nb, int li, int lj, int lk, int64_t cell,
                                             const uint8_t* __restrict__ amask, const int32_t* __restrict__ voff,
                                             int32_t* __restrict__ faces, int64_t* __restrict__ face_cell, int64_t face_cap,
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
      const int64_t o = mts_row(nb, li + (int)(oc & 1u), lj + (int)((oc >> 1) & 1u), lk + (int)(oc >> 2));
      idx[c] = o < 0 ? -1 : voff[o] + __popc((unsigned)amask[o] & ((1u << sl) - 1u));    // -1: the caller broke its guarantee
    }
    if (f < face_cap) {
      faces[3 * f] = idx[0];
      faces[3 * f + 1] = idx[1];
      faces[3 * f + 2] = idx[2];
      if (face_cell) face_cell[f] = cell;
    }
    ++f;
  }
}

__global__ __launch_bounds__(MTS_BLOCK) void k_mts_emit(const float* __restrict__ values, const int32_t* __restrict__ coords,
                                                        const uint8_t* __restrict__ cell_active, int64_t S, MtsDims d, MtGrid g,
                                                        const int32_t* __restrict__ table, const uint8_t* __restrict__ amask,
                                                        const int32_t* __restrict__ voff, const int32_t* __restrict__ toff,
                                                        const int32_t* __restrict__ partial, float* __restrict__ verts,
                                                        int64_t vert_cap, int32_t* __restrict__ faces, int64_t face_cap,
                                                        int64_t* __restrict__ vert_key, int64_t* __restrict__ face_cell) {
  __shared__ int nb[8];
  const int s = blockIdx.x, t = threadIdx.x;
  if (partial[2 * s] == 0) return;                          // no vertex, so no face either; uniform over the workgroup
  const int bi = coords[3 * s], bj = coords[3 * s + 1], bk = coords[3 * s + 2];
  mts_neighbours(d, table, s, bi, bj, bk, nb);
  __syncthreads();
  const int64_t row = (int64_t)s * MTS_BLOCK + t;
  const unsigned am = amask[row];
  if (am == 0u) return;
  const int li = t >> 6, lj = (t >> 3) & 7, lk = t & 7;
  const int gi = 8 * bi + li, gj = 8 * bj + lj, gk = 8 * bk + lk;
  const unsigned em = exist_mask(gi + 1 < g.nx, gj + 1 < g.ny, gk + 1 < g.nz);
  float v[8];
  v[0] = values[row];
#pragma unroll
  for (int c = 1; c < 8; ++c) {
    const int code = kSlotCode[c - 1];
    const int64_t o = ((em >> c) & 1u) ? mts_row(nb, li + (code & 1), lj + ((code >> 1) & 1), lk + (code >> 2)) : -1;
    v[c] = o >= 0 ? values[o] : v[0];
  }
  const int64_t p = ((int64_t)gi * g.ny + gj) * g.nz + gk;   // the dense linear index: the keys
  int64_t vi = voff[row];
#pragma unroll
  for (int sl = 0; sl < 7; ++sl) {
    if ((am >> sl) & 1u) {
      float pos[3];
      mt_vertex(g, gi, gj, gk, kSlotCode[sl], v[0], v[sl + 1], pos);
      if (vi < vert_cap) {
#pragma unroll
        for (int q = 0; q < 3; ++q) verts[3 * vi + q] = pos[q];
        if (vert_key) vert_key[vi] = 7 * p + sl;
      }
      ++vi;
    }
  }
  if (em == 0xffu && cell_active[s] != 0) {
    unsigned cm = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) cm |= mt_inside(v[c], g.iso) << c;
    int64_t f = toff[row];
    mts_emit_tet<0>(cm, nb, li, lj, lk, p, amask, voff, faces, face_cell, face_cap, f);
    mts_emit_tet<1>(cm, nb, li, lj, lk, p, amask, voff, faces, face_cell, face_cap, f);
    mts_emit_tet<2>(cm, nb, li, lj, lk, p, amask, voff, faces, face_cell, face_cap, f);
    mts_emit_tet<3>(cm, nb, li, lj, lk, p, amask, voff, faces, face_cell, face_cap, f);
    mts_emit_tet<4>(cm, nb, li, lj, lk, p, amask, voff, faces, face_cell, face_cap, f);
    mts_emit_tet<5>(cm, nb, li, lj, lk, p, amask, voff, faces, face_cell, face_cap, f);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct MtsLayout {
  int64_t n_rows, n_bricks;
  int64_t table, cnt, off, amask, partial, scan, scan_bytes, bytes;      // byte offsets into the workspace
};

MtsLayout mts_layout(const MtsDims& d, int64_t S) {
  MtsLayout L;
  L.n_rows = S * MTS_BLOCK;
  L.n_bricks = (int64_t)d.bx * d.by * d.bz;
  L.table = 0;
  L.cnt = L.table + iso_align16(4 * L.n_bricks);
  L.off = L.cnt + iso_align16(8 * L.n_rows);
  L.amask = L.off + iso_align16(8 * L.n_rows);
  L.partial = L.amask + iso_align16(L.n_rows);
  L.scan = L.partial + iso_align16(8 * S);
  L.scan_bytes = iso_prefix_sum_workspace_bytes(L.n_rows, 2);
  L.bytes = L.scan + iso_align16(L.scan_bytes);
  return L;
}

int mts_check(const char* fn, int nx, int ny, int nz, int64_t S, float iso) {
  ISO_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, ISO_ERR_INVALID, "%s: a grid needs at least 2 points per axis, got %d x %d x %d", fn,
              nx, ny, nz);
  ISO_REQUIRE(nx <= MTS_MAX_N && ny <= MTS_MAX_N && nz <= MTS_MAX_N, ISO_ERR_UNSUPPORTED,
              "%s: at most %d points per axis, got %d x %d x %d", fn, MTS_MAX_N, nx, ny, nz);
  ISO_REQUIRE(S >= 1, ISO_ERR_INVALID, "%s: the brick list is empty (%lld)", fn, (long long)S);
  ISO_REQUIRE(S * MTS_BLOCK < (1ll << 31), ISO_ERR_UNSUPPORTED, "%s: %lld bricks; the limit is 2^31 - 1 points in all", fn,
              (long long)S);
  ISO_REQUIRE(fabsf(iso) <= FLT_MAX, ISO_ERR_INVALID, "%s: the level must be finite", fn);
  return ISO_OK;
}

}  // namespace

extern "C" int64_t iso_meshextract_sparse_workspace_bytes(int nx, int ny, int nz, int64_t n_bricks) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > MTS_MAX_N || ny > MTS_MAX_N || nz > MTS_MAX_N) return 0;
  if (n_bricks < 1 || n_bricks * MTS_BLOCK >= (1ll << 31)) return 0;
  return mts_layout(mts_dims(nx, ny, nz), n_bricks).bytes;
}

extern "C" int iso_meshextract_sparse_count(const float* values, const int32_t* coords, const uint8_t* cell_active,
                                             int64_t n_bricks, int nx, int ny, int nz, float iso, uint8_t* need, int64_t* totals,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "iso_meshextract_sparse_count";
  const int rc = mts_check(fn, nx, ny, nz, n_bricks, iso);
  if (rc != ISO_OK) return rc;
  ISO_REQUIRE(values && coords && cell_active && need && totals && workspace, ISO_ERR_INVALID, "%s: null pointer", fn);
  const MtsDims d = mts_dims(nx, ny, nz);
  const MtsLayout L = mts_layout(d, n_bricks);
  ISO_REQUIRE(workspace_bytes >= L.bytes, ISO_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld)", fn,
              (long long)workspace_bytes, (long long)L.bytes);
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "%s: the workspace must be 16-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* table = (int32_t*)(ws + L.table);
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int32_t* partial = (int32_t*)(ws + L.partial);
  hipLaunchKernelGGL(k_mts_fill, dim3(iso_stream_grid(L.n_bricks, 256)), dim3(256), 0, s, table, L.n_bricks, -1);
  hipLaunchKernelGGL(k_mts_table, dim3(iso_div_up(n_bricks, 256)), dim3(256), 0, s, coords, n_bricks, d, table);
  hipLaunchKernelGGL(k_mts_classify, dim3((unsigned)n_bricks), dim3(MTS_BLOCK), 0, s, values, coords, cell_active, n_bricks, d,
                     iso, table, (uint8_t*)(ws + L.amask), cnt, partial, need);
  hipLaunchKernelGGL(k_mts_totals, dim3(1), dim3(1024), 0, s, partial, need, coords, n_bricks, d, totals);
  ISO_CHECK_LAUNCH(fn);
  return iso_prefix_sum(cnt, (int32_t*)(ws + L.off), L.n_rows, 2, L.n_rows, ws + L.scan, L.scan_bytes, stream);
}

extern "C" int iso_meshextract_sparse_emit(const float* values, const int32_t* coords, const uint8_t* cell_active,
                                            int64_t n_bricks, int nx, int ny, int nz, float ox, float oy, float oz, float sx,
                                            float sy, float sz, float iso, const int64_t* totals, float* verts,
                                            int64_t vert_capacity, int32_t* faces, int64_t face_capacity, int64_t* vert_key,
                                            int64_t* face_cell, const void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "iso_meshextract_sparse_emit";
  const int rc = mts_check(fn, nx, ny, nz, n_bricks, iso);
  if (rc != ISO_OK) return rc;
  ISO_REQUIRE(fabsf(ox) <= FLT_MAX && fabsf(oy) <= FLT_MAX && fabsf(oz) <= FLT_MAX, ISO_ERR_INVALID, "%s: the origin must be finite", fn);
  ISO_REQUIRE(sx > 0.f && sy > 0.f && sz > 0.f && sx <= FLT_MAX && sy <= FLT_MAX && sz <= FLT_MAX, ISO_ERR_INVALID,
              "%s: the spacing must be positive and finite", fn);
  ISO_REQUIRE(values && coords && cell_active && totals && workspace, ISO_ERR_INVALID, "%s: null pointer", fn);
  ISO_REQUIRE(vert_capacity >= 0 && face_capacity >= 0, ISO_ERR_INVALID, "%s: negative capacity", fn);
  const MtsDims d = mts_dims(nx, ny, nz);
  const MtsLayout L = mts_layout(d, n_bricks);
  ISO_REQUIRE(workspace_bytes >= L.bytes, ISO_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld)", fn,
              (long long)workspace_bytes, (long long)L.bytes);
  hipStream_t s = (hipStream_t)stream;
  // the one host read of the entry: the counted totals, to refuse a list that left the grid and outputs that are too small
  int64_t tot[4] = {0, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(tot, totals, sizeof(tot), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  ISO_REQUIRE(e == hipSuccess, ISO_ERR_LAUNCH, "%s: reading the totals failed: %s", fn, hipGetErrorString(e));
  ISO_REQUIRE(tot[3] == 0, ISO_ERR_INVALID, "%s: %lld bricks of the list lie outside the grid of %d x %d x %d bricks", fn,
              (long long)tot[3], d.bx, d.by, d.bz);
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
  hipLaunchKernelGGL(k_mts_emit, dim3((unsigned)n_bricks), dim3(MTS_BLOCK), 0, s, values, coords, cell_active, n_bricks, d, g,
                     (const int32_t*)(ws + L.table), (const uint8_t*)(ws + L.amask), off, off + L.n_rows,
                     (const int32_t*)(ws + L.partial), verts, vert_capacity, faces, face_capacity, vert_key, face_cell);
  ISO_CHECK_LAUNCH(fn);
  return ISO_OK;
}
