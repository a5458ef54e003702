// Poisson-disk elimination on the cell grid of frnn.hip, written for gfx950: drop samples of a cloud until no two are
// closer than a radius (include/isopoints.h section L for the call sites and the definition).
//
// Definition.  Samples i and j of a cloud CONFLICT iff d2(i, j) <= r2, with d2 = rec_d2() of cell_grid.h (f32, no
// contraction) and r2 = r * r in f32.  Sample s is KEPT iff no kept sample j < s conflicts with it; a sample that is invalid
// on entry is removed and blocks nobody.  That is serial dart throwing in index order: an exact integer result.
//
// Parallel form.  One state byte per sample: UNDECIDED, KEEP or REMOVED.  A round visits every UNDECIDED sample s and reads
// the state of every conflicting j < s: any KEEP makes s REMOVED; else any UNDECIDED leaves s as it is; else s becomes KEEP.
// Why the result is the serial one whatever the launch shape, the timing or the number of rounds per launch:
//   * a state only ever moves from UNDECIDED to a final value, and only the lane that owns the sample writes it;
//   * s is finalised only from FINAL states of lower indices: REMOVED needs one conflicting KEEP below s, KEEP needs every
//     conflicting sample below s REMOVED.  By induction on the index a final state is the serial state: the lowest valid
//     sample has nothing below it and is kept; if every final state below s is the serial one, a conflicting KEEP below s
//     is a kept sample of the serial order (s is removed there too), and all conflicting samples below s REMOVED means the
//     serial order keeps s;
//   * so a round may update the bytes in place.  A stale read (another workgroup's store not yet visible: the vector L1 is
//     never refreshed by another CU's stores, the XCDs' L2s are not coherent inside a launch) shows UNDECIDED where a final
//     value stands, never a wrong final value, and UNDECIDED only leaves s open: the decision is delayed, not changed;
//   * a launch boundary makes every earlier store visible, so each round finalises at least the lowest UNDECIDED sample of
//     every cloud: the loop ends, after at most as many rounds as the longest chain of conflicts has links.
// The fixed point is unique, hence two runs give the same bytes.
//
//   k_disk_round   : one lane per record of the cloud's own grid (sorted by cell: neighbouring lanes walk neighbouring
//                    cells).  An UNDECIDED lane walks the shells of its cell -- visit_block27, then visit_shell_lane -- up
//                    to the first shell rho with ring_reach(rho, cell) >= r (the build never makes cells finer than r / 2
//                    but may make them smaller than r) and stops early at the first conflicting KEEP.  The lanes still
//                    UNDECIDED are counted per workgroup and added to a device counter; a launch whose predecessor left 0
//                    returns at once.
//   k_disk_select  : the stable compaction of the KEEP bytes per cloud, in index order: tile counts, one scan of the tile
//                    counts per cloud, then each tile's own scan.  Integer work only.
#include <float.h>
#include "cell_grid.h"

#pragma clang fp contract(off)

namespace {

constexpr uint8_t kUndecided = 0, kKeep = 1, kRemoved = 2;
constexpr int kRoundBlock = 256;
constexpr int kTile = 2048;          // samples per workgroup of the compaction: 256 threads x 8 in index order
constexpr int kCounters = 4;         // three rotating round counters (read / add / zeroed for the next round) + padding

struct DiskWorkspace {
  float4* xyzi;        // (N,P) records of the grid
  uint8_t* state;      // (N,P) by ORIGINAL index
  int32_t* counters;   // kCounters
  int32_t* tile_cnt;   // (N, tiles) KEEP bytes per tile, then their exclusive scan
  int32_t* total;      // (N) KEEP bytes per cloud
};

inline int64_t disk_tiles(int64_t p) { return (p + kTile - 1) / kTile; }

inline DiskWorkspace disk_carve(void* ws, int n, int64_t p) {
  DiskWorkspace w;
  char* c = (char*)ws;
  w.xyzi = reinterpret_cast<float4*>(c);
  c += 16 * (int64_t)n * p;
  w.state = reinterpret_cast<uint8_t*>(c);
  c += iso_align16((int64_t)n * p);
  w.counters = reinterpret_cast<int32_t*>(c);
  c += iso_align16(kCounters * 4);
  w.tile_cnt = reinterpret_cast<int32_t*>(c);
  c += iso_align16((int64_t)n * disk_tiles(p) * 4);
  w.total = reinterpret_cast<int32_t*>(c);
  return w;
}

// rows beyond the cloud's length and rows the caller marks invalid are REMOVED from the start
__global__ __launch_bounds__(256) void k_disk_init(const int64_t* __restrict__ lengths, const uint8_t* __restrict__ valid,
                                                    uint8_t* __restrict__ state, int32_t* __restrict__ counters,
                                                    int64_t p) {
  const int n = blockIdx.y;
  const int64_t len = lengths ? lengths[n] : p;
  if (blockIdx.x == 0 && n == 0 && threadIdx.x < kCounters) counters[threadIdx.x] = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = (int64_t)n * p + i;
    state[r] = (i < len && (!valid || valid[r])) ? kUndecided : kRemoved;
  }
}

// Round number `round` of the call: reads counters[(round + 2) % 3] (what the previous round left UNDECIDED), adds to
// counters[round % 3] (zeroed by the previous round, or by k_disk_init) and zeroes counters[(round + 1) % 3] for its successor.
__global__ __launch_bounds__(kRoundBlock) void k_disk_round(const float4* __restrict__ xyzi,
                                                            const int64_t* __restrict__ lengths,
                                                            const int32_t* __restrict__ off,
                                                            const float* __restrict__ params,
                                                            const float* __restrict__ radius, uint8_t* state,
                                                            int32_t* counters, int round, int64_t p, int64_t g_stride) {
  __shared__ int s_open[kRoundBlock / 64];
  const int n = blockIdx.y;
  if (blockIdx.x == 0 && n == 0 && threadIdx.x == 0) counters[(round + 1) % 3] = 0;
  if (round > 0 && counters[(round + 2) % 3] == 0) return;
  const int64_t len = lengths ? lengths[n] : p;
  const float4* s4 = xyzi + (int64_t)n * p;
  uint8_t* st = state + (int64_t)n * p;
  const Grid3 g = grid3_load(params, n);
  const int32_t* offn = off + (int64_t)n * g_stride;
  const float r = radius[n];
  const float r2 = r * r;
  int open = 0;
  for (int64_t t = (int64_t)blockIdx.x * kRoundBlock + threadIdx.x; t < len; t += (int64_t)gridDim.x * kRoundBlock) {
    const float4 me = s4[t];
    const int s = __float_as_int(me.w);
    if (st[s] != kUndecided) continue;
    bool kept_below = false, open_below = false;
    auto scan = [&](int64_t i0, int64_t i1) {
      if (kept_below) return;
      scan_run2(s4, i0, i1, me.x, me.y, me.z, [&](float d2, int oi) {
        if (oi < s && d2 <= r2) {
          const uint8_t o = st[oi];
          kept_below |= (o == kKeep);
          open_below |= (o == kUndecided);
        }
      });
    };
    const QueryCell c = query_cell(g, me.x, me.y, me.z);
    int rho = c.rho0;
    bool reached = false;
    if (c.rho0 == 0 && c.span >= 1) {
      visit_block27(g, offn, len, c, scan);
      reached = ring_reach(1, g.cell) >= r;
      rho = 2;
    }
    for (; rho <= c.span && !reached && !kept_below; ++rho) {
      visit_shell_lane(g, offn, len, c, rho, scan);
      reached = ring_reach(rho, g.cell) >= r;
    }
    if (kept_below) st[s] = kRemoved;
    else if (!open_below) st[s] = kKeep;
    else ++open;
  }
  // the lanes left open, one add per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o);
  if ((threadIdx.x & 63) == 0) s_open[threadIdx.x >> 6] = open;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < kRoundBlock / 64; ++w) tot += s_open[w];
    if (tot) atomicAdd(&counters[round % 3], tot);
  }
}

__global__ void k_disk_left(const int32_t* __restrict__ counters, int last_round, int32_t* __restrict__ left) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *left = counters[last_round % 3];
}

// the KEEP bytes of the 8 consecutive samples of a thread, as bits
__device__ __forceinline__ int disk_thread_bits(const uint8_t* __restrict__ st, int64_t base, int64_t p) {
  int bits = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t i = base + k;
    if (i < p && st[i] == kKeep) bits |= 1 << k;
  }
  return bits;
}

__global__ __launch_bounds__(256) void k_disk_tile_count(const uint8_t* __restrict__ state, int32_t* __restrict__ tile_cnt,
                                                          int64_t p, int64_t tiles) {
  __shared__ int lds[4];
  const int n = blockIdx.y;
  const uint8_t* st = state + (int64_t)n * p;
  for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    int total;
    iso_block_excl_scan<4>(__popc(disk_thread_bits(st, tl * kTile + threadIdx.x * 8, p)), total, lds);
    if (threadIdx.x == 0) tile_cnt[(int64_t)n * tiles + tl] = total;
  }
}

// tile_cnt[n] -> its exclusive scan in place, total[n], kept_out[n] = min(total, s_out): one workgroup per cloud
__global__ __launch_bounds__(256) void k_disk_tile_scan(int32_t* __restrict__ tile_cnt, int32_t* __restrict__ total_out,
                                                         int64_t* __restrict__ kept_out, int64_t tiles, int64_t s_out) {
  __shared__ int lds[4];
  const int n = blockIdx.x;
  int32_t* tc = tile_cnt + (int64_t)n * tiles;
  int carry = 0;
  for (int64_t t0 = 0; t0 < tiles; t0 += 256) {
    const int64_t i = t0 + threadIdx.x;
    const int v = i < tiles ? tc[i] : 0;
    int total;
    const int ex = iso_block_excl_scan<4>(v, total, lds);
    if (i < tiles) tc[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    total_out[n] = carry;
    kept_out[n] = (int64_t)carry < s_out ? (int64_t)carry : s_out;
  }
}

// sel_out[n, k] = the index of the k-th KEEP sample of cloud n for k < min(total, s_out), -1 beyond; mask_out = KEEP or not
__global__ __launch_bounds__(256) void k_disk_select(const uint8_t* __restrict__ state, const int32_t* __restrict__ tile_off,
                                                      const int32_t* __restrict__ total, uint8_t* __restrict__ mask_out,
                                                      int32_t* __restrict__ sel_out, int64_t p, int64_t tiles,
                                                      int64_t s_out) {
  __shared__ int lds[4];
  const int n = blockIdx.y;
  const uint8_t* st = state + (int64_t)n * p;
  int32_t* sel = sel_out + (int64_t)n * s_out;
  for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const int64_t base = tl * kTile + threadIdx.x * 8;
    const int bits = disk_thread_bits(st, base, p);
    int total;
    int64_t at = (int64_t)tile_off[(int64_t)n * tiles + tl] + iso_block_excl_scan<4>(__popc(bits), total, lds);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = base + k;
      if (i < p) {
        const bool keep = (bits >> k) & 1;
        if (mask_out) mask_out[(int64_t)n * p + i] = keep ? 1 : 0;
        if (keep) {
          if (at < s_out) sel[at] = (int32_t)i;
          ++at;
        }
      }
    }
  }
  const int64_t kept = total[n];
  for (int64_t k = kept + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < s_out; k += (int64_t)gridDim.x * blockDim.x)
    sel[k] = -1;
}

// clouds without rows: nothing is kept
__global__ void k_disk_none(int32_t* __restrict__ sel_out, int64_t* __restrict__ kept_out, int n_clouds, int64_t n_sel) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = i0; i < n_clouds; i += (int64_t)gridDim.x * blockDim.x) kept_out[i] = 0;
  for (int64_t i = i0; i < n_sel; i += (int64_t)gridDim.x * blockDim.x) sel_out[i] = -1;
}

// radius_out[n] = sqrt(A_n / (3 S)) with A_n the f64 sum of the mesh's f32 face areas: a thread adds its faces in index
// order (stride 256), the 256 sums are added in thread order.  A mesh without area gets 0.
__global__ __launch_bounds__(256) void k_disk_area_radius(const float* __restrict__ areas, const int64_t* __restrict__ first,
                                                           const int64_t* __restrict__ len, int64_t n_tris,
                                                           int64_t n_samples, float* __restrict__ radius_out) {
  __shared__ double s_sum[256];
  const int n = blockIdx.x;
  int64_t f0 = first[n], f1 = first[n] + len[n];
  if (f0 < 0) f0 = 0;
  if (f1 > n_tris) f1 = n_tris;
  double a = 0.0;
  for (int64_t f = f0 + threadIdx.x; f < f1; f += 256) a += (double)areas[f];
  s_sum[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double A = 0.0;
    for (int k = 0; k < 256; ++k) A += s_sum[k];
    const bool ok = A > 0.0 && A < (double)FLT_MAX;
    radius_out[n] = ok ? (float)sqrt(A / (3.0 * (double)n_samples)) : 0.f;
  }
}

int disk_check(const char* fn, int n_clouds, int64_t p_stride, const void* workspace, int64_t workspace_bytes) {
  ISO_REQUIRE(n_clouds >= 0 && p_stride >= 0, ISO_ERR_INVALID, "%s: bad sizes", fn);
  ISO_REQUIRE((int64_t)n_clouds * p_stride < 0x7fffffff, ISO_ERR_UNSUPPORTED, "%s: 32-bit sample indices (N * P < 2^31 - 1)", fn);
  if (n_clouds == 0 || p_stride == 0) return ISO_OK;
  ISO_REQUIRE(workspace && workspace_bytes >= iso_disk_workspace_bytes(n_clouds, p_stride), ISO_ERR_WORKSPACE,
              "%s: workspace too small", fn);
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0, ISO_ERR_INVALID, "%s: workspace must be 16-B aligned", fn);
  return ISO_OK;
}

}  // namespace

// workspace of the iso_disk_* calls: [records: N*P float4][state: N*P bytes][counters][tile counts: N * tiles][totals: N]
extern "C" int64_t iso_disk_workspace_bytes(int n_clouds, int64_t p_stride) {
  if (n_clouds < 0) n_clouds = 0;
  if (p_stride < 0) p_stride = 0;
  const int64_t np = (int64_t)n_clouds * p_stride;
  return 16 * np + iso_align16(np) + iso_align16(kCounters * 4) + iso_align16((int64_t)n_clouds * disk_tiles(p_stride) * 4) +
         iso_align16((int64_t)n_clouds * 4) + 16;
}

extern "C" int iso_disk_begin(const float* sorted_points, const int32_t* sorted_idx, const int64_t* lengths,
                              const uint8_t* valid, int n_clouds, int64_t p_stride, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  const int rc = disk_check("iso_disk_begin", n_clouds, p_stride, workspace, workspace_bytes);
  if (rc != ISO_OK || n_clouds == 0 || p_stride == 0) return rc;
  ISO_REQUIRE(sorted_points && sorted_idx, ISO_ERR_INVALID, "iso_disk_begin: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const DiskWorkspace w = disk_carve(workspace, n_clouds, p_stride);
  pack_xyzi(sorted_points, sorted_idx, lengths, n_clouds, p_stride, w.xyzi, s);
  hipLaunchKernelGGL(k_disk_init, dim3(iso_capped_grid(p_stride, 256, 2048), n_clouds), dim3(256), 0, s, lengths, valid,
                     w.state, w.counters, p_stride);
  ISO_CHECK_LAUNCH("iso_disk_begin");
  return ISO_OK;
}

extern "C" int iso_disk_rounds(const int64_t* lengths, const int32_t* off, const float* grid_params, const float* radius,
                               int n_clouds, int64_t p_stride, int64_t g_stride, int first_round, int n_rounds,
                               int32_t* left, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = disk_check("iso_disk_rounds", n_clouds, p_stride, workspace, workspace_bytes);
  if (rc != ISO_OK) return rc;
  ISO_REQUIRE(first_round >= 0 && n_rounds >= 1 && first_round <= 0x7fffffff - n_rounds - 2 && g_stride >= 0,
              ISO_ERR_INVALID, "iso_disk_rounds: bad round numbers or grid stride");
  ISO_REQUIRE(left, ISO_ERR_INVALID, "iso_disk_rounds: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_clouds == 0 || p_stride == 0) {
    iso_zero_words(left, 1, s);
    ISO_CHECK_LAUNCH("iso_disk_rounds");
    return ISO_OK;
  }
  ISO_REQUIRE(off && grid_params && radius, ISO_ERR_INVALID, "iso_disk_rounds: null pointer");
  const DiskWorkspace w = disk_carve(workspace, n_clouds, p_stride);
  const int gx = iso_capped_grid(p_stride, kRoundBlock, 4096);
  for (int k = 0; k < n_rounds; ++k)
    hipLaunchKernelGGL(k_disk_round, dim3(gx, n_clouds), dim3(kRoundBlock), 0, s, w.xyzi, lengths, off, grid_params, radius,
                       w.state, w.counters, first_round + k, p_stride, g_stride);
  hipLaunchKernelGGL(k_disk_left, dim3(1), dim3(64), 0, s, w.counters, first_round + n_rounds - 1, left);
  ISO_CHECK_LAUNCH("iso_disk_rounds");
  return ISO_OK;
}

extern "C" int iso_disk_select(int n_clouds, int64_t p_stride, int64_t s_out, uint8_t* mask_out, int32_t* sel_out,
                               int64_t* kept_out, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = disk_check("iso_disk_select", n_clouds, p_stride, workspace, workspace_bytes);
  if (rc != ISO_OK) return rc;
  ISO_REQUIRE(s_out >= 0 && (int64_t)n_clouds * s_out < 0x7fffffff, ISO_ERR_INVALID, "iso_disk_select: bad s_out");
  if (n_clouds == 0) return ISO_OK;
  ISO_REQUIRE(kept_out && (sel_out || s_out == 0), ISO_ERR_INVALID, "iso_disk_select: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (p_stride == 0) {
    hipLaunchKernelGGL(k_disk_none, dim3(iso_capped_grid((int64_t)n_clouds * s_out, 256, 2048)), dim3(256), 0, s, sel_out,
                       kept_out, n_clouds, (int64_t)n_clouds * s_out);
    ISO_CHECK_LAUNCH("iso_disk_select");
    return ISO_OK;
  }
  const DiskWorkspace w = disk_carve(workspace, n_clouds, p_stride);
  const int64_t tiles = disk_tiles(p_stride);
  const int gx = (int)(tiles < 2048 ? tiles : 2048);
  hipLaunchKernelGGL(k_disk_tile_count, dim3(gx, n_clouds), dim3(256), 0, s, w.state, w.tile_cnt, p_stride, tiles);
  hipLaunchKernelGGL(k_disk_tile_scan, dim3(n_clouds), dim3(256), 0, s, w.tile_cnt, w.total, kept_out, tiles, s_out);
  hipLaunchKernelGGL(k_disk_select, dim3(gx, n_clouds), dim3(256), 0, s, w.state, w.tile_cnt, w.total, mask_out, sel_out,
                     p_stride, tiles, s_out);
  ISO_CHECK_LAUNCH("iso_disk_select");
  return ISO_OK;
}

extern "C" int iso_disk_area_radius(const float* areas, const int64_t* tris_first, const int64_t* tris_len, int n_meshes,
                                    int64_t n_tris, int64_t n_samples, float* radius_out, void* stream) {
  ISO_REQUIRE(n_meshes >= 0 && n_tris >= 0 && n_samples >= 1, ISO_ERR_INVALID, "iso_disk_area_radius: bad sizes");
  if (n_meshes == 0) return ISO_OK;
  ISO_REQUIRE(tris_first && tris_len && radius_out && (areas || n_tris == 0), ISO_ERR_INVALID,
              "iso_disk_area_radius: null pointer");
  hipLaunchKernelGGL(k_disk_area_radius, dim3(n_meshes), dim3(256), 0, (hipStream_t)stream, areas, tris_first, tris_len,
                     n_tris, n_samples, radius_out);
  ISO_CHECK_LAUNCH("iso_disk_area_radius");
  return ISO_OK;
}
