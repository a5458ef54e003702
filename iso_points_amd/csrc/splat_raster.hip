// EWA surface splatting for gfx950, stage 2 of 6: tile binning and the per-tile raster.
// (set-up: splat.hip -> here -> splat_composite.hip; backward: splat_backward.hip, splat_median.hip; the reference's
// coarse / fine interface: splat_bins.hip.  What a pixel does is in splat_pixel.h, its K-best list in kbest.h.)
//
// Reference semantics
//   forward  : _C.splat_points -> RasterizePoints{Naive,Coarse,Fine}
//              DSS/csrc/rasterize_points.cu:65-211,293-430,506-596 (CPU twin
//              rasterize_points_cpu.cpp:27-144)
//
// Design (MI355X): the reference bins 512-point chunks into <=21x21 bins with 64
// workgroups and then lets every pixel scan all M = max(1e4,P) slots of its
// bin (an N*B*B*M int table: 4 GB at 1M points).  Here points are binned into
// 16x16-pixel tiles by a count -> scan -> fill counting sort (one int per
// point-tile pair), and one 256-lane workgroup per tile streams its candidate
// list through LDS in 256-entry chunks (every lane reads the same LDS word:
// broadcast, conflict free) while each lane keeps the K front-most (z, idx)
// hits of its own pixel in registers.  4096 tiles at 512^2 x 4 views fill the
// 256 CUs 16 times over.  The K-best rule is the reference CPU's
// lexicographic (z, idx) order, so per-pixel index lists are deterministic and
// bit-identical to the compiled reference no matter in which order the atomics
// of the fill pass land.
#include "splat_pixel.h"

#pragma clang fp contract(off)

namespace {

template <bool FILL>
__global__ void k_bin(const float* __restrict__ pts, const float* __restrict__ radii,
                      const int64_t* __restrict__ first, const int64_t* __restrict__ num, Frame F,
                      int ty_begin, int ty_end,
                      int32_t* __restrict__ tile_cnt,
                      const int32_t* __restrict__ tile_off, int32_t* __restrict__ pairs,
                      int64_t capacity, int32_t* __restrict__ overflow) {
  const int n = blockIdx.y;
  const int64_t len = num[n], base = first[n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + i;
    const float z = pts[p * 3 + 2];
    if (!(z >= 0.f)) continue;  // behind the camera (rasterize_points.cu:87-88) or NaN
    int x0, x1, y0, y1;
    if (!pixel_range(pts[p * 3], radii[p * 2], F.W, F.ex, F.m, x0, x1)) continue;
    if (!pixel_range(pts[p * 3 + 1], radii[p * 2 + 1], F.H, F.ey, F.m, y0, y1)) continue;
    for (int ty = max(y0 / TILE, ty_begin); ty <= min(y1 / TILE, ty_end - 1); ++ty)
      for (int tx = x0 / TILE; tx <= x1 / TILE; ++tx) {
        const int tile = (n * F.Ty + ty) * F.Tx + tx;
        const int slot = atomicAdd(&tile_cnt[tile], 1);
        if (FILL) {
          const int64_t dst = (int64_t)tile_off[tile] + slot;
          if (dst < capacity) pairs[dst] = (int32_t)p;
          else *overflow = 1;
        }
      }
  }
}

// Same binning with the per-tile counters privatised in LDS (one view's T*T tiles fit for S <= 1024):
// a workgroup walks kBinChunk consecutive points, counts them per tile in LDS, reserves one range per
// touched tile with a single global atomic and (FILL) hands out the slots from LDS.  The hot tiles on
// a silhouette otherwise take thousands of same-address global atomics.
// The work items of the raster pass (tile_items_body, below) only need the tile offsets, not the filled pair list: the
// FILL launch carries them as one more workgroup (blockIdx = (gridDim.x - 1, 0)) instead of a single-workgroup launch
// of its own between the fill and the raster (14 us of the cfg-3a cycle).
struct TileItemsJob {          // what k_tile_items takes; items == null: no job
  int ty_rows, n_clouds, max_slots, target_items;
  int4* items; int4* heavy; int32_t* counters;
};
__device__ void tile_items_body(const int32_t* __restrict__ tile_off, Frame F, int ty_begin, int ty_rows, int n_clouds,
                                int max_slots, int target_items, int4* __restrict__ items, int4* __restrict__ heavy,
                                int32_t* __restrict__ counters);
constexpr int kBinChunk = 2048;      // rows per workgroup: 8 per thread -- with 8192 a 512^2 x 4 job was 245 workgroups of 32 sequential rows per thread, latency bound
template <bool FILL>
__global__ __launch_bounds__(256) void k_bin_lds(const float* __restrict__ pts, const float* __restrict__ radii,
                                                 const int64_t* __restrict__ first, const int64_t* __restrict__ num,
                                                 Frame F, int ty_begin, int ty_end,
                                                 int32_t* __restrict__ tile_cnt, const int32_t* __restrict__ tile_off,
                                                 int32_t* __restrict__ pairs, int64_t capacity,
                                                 int32_t* __restrict__ overflow, TileItemsJob job) {
  extern __shared__ int lh[];          // Tx*Ty
  if (FILL && job.items && blockIdx.x == gridDim.x - 1) {           // the extra workgroup(s) of the launch
    if (blockIdx.y == 0)
      tile_items_body(tile_off, F, ty_begin, job.ty_rows, job.n_clouds, job.max_slots, job.target_items, job.items,
                      job.heavy, job.counters);
    return;
  }
  const int TT = F.Tx * F.Ty;
  const int n = blockIdx.y;
  const int64_t len = num[n], base = first[n];
  const int64_t i0 = (int64_t)blockIdx.x * kBinChunk;
  if (i0 >= len) return;
  const int64_t i1 = min(len, i0 + kBinChunk);
  for (int t = threadIdx.x; t < TT; t += blockDim.x) lh[t] = 0;
  __syncthreads();
  auto walk = [&](auto&& visit) {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
      const int64_t p = base + i;
      const float z = pts[p * 3 + 2];
      if (!(z >= 0.f)) continue;  // behind the camera (rasterize_points.cu:87-88) or NaN
      int x0, x1, y0, y1;
      if (!pixel_range(pts[p * 3], radii[p * 2], F.W, F.ex, F.m, x0, x1)) continue;
      if (!pixel_range(pts[p * 3 + 1], radii[p * 2 + 1], F.H, F.ey, F.m, y0, y1)) continue;
      for (int ty = max(y0 / TILE, ty_begin); ty <= min(y1 / TILE, ty_end - 1); ++ty)
        for (int tx = x0 / TILE; tx <= x1 / TILE; ++tx) visit(ty * F.Tx + tx, p);
    }
  };
  walk([&](int t, int64_t) { atomicAdd(&lh[t], 1); });
  __syncthreads();
  for (int t = threadIdx.x; t < TT; t += blockDim.x) {
    const int c = lh[t];
    if (c) {
      const int b = atomicAdd(&tile_cnt[n * TT + t], c);
      if (FILL) lh[t] = b;
    }
  }
  if (!FILL) return;
  __syncthreads();
  walk([&](int t, int64_t p) {
    const int slot = atomicAdd(&lh[t], 1);
    const int64_t dst = (int64_t)tile_off[n * TT + t] + slot;
    if (dst < capacity) pairs[dst] = (int32_t)p;
    else *overflow = 1;
  });
}

// returns true when the launch carried `job` (the caller then issues no k_tile_items launch)
template <bool FILL>
bool launch_bin(const float* points, const float* radii, const int64_t* first_idx, const int64_t* num_pts,
                int n_clouds, int64_t max_pts, Frame F, int ty0, int ty1, int32_t* tile_cnt,
                const int32_t* tile_off, int32_t* pairs, int64_t capacity, int32_t* overflow, hipStream_t s,
                TileItemsJob job = TileItemsJob{0, 0, 0, 0, nullptr, nullptr, nullptr}) {
  if (F.Tx * F.Ty <= 4096) {
    const bool carry = FILL && job.items != nullptr;
    hipLaunchKernelGGL(k_bin_lds<FILL>, dim3(iso_div_up(max_pts, kBinChunk) + (carry ? 1 : 0), n_clouds), dim3(256),
                       (size_t)F.Tx * F.Ty * sizeof(int), s, points, radii, first_idx, num_pts, F, ty0, ty1, tile_cnt,
                       tile_off, pairs, capacity, overflow, job);
    return carry;
  } else {
    int gx = iso_div_up(max_pts, 256); if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(k_bin<FILL>, dim3(gx, n_clouds), dim3(256), 0, s, points, radii, first_idx, num_pts, F,
                       ty0, ty1, tile_cnt, tile_off, pairs, capacity, overflow);
    return false;
  }
}

// How the hits of a chunk of 256 candidates reach the pixels ("candidate parallel"): thread t walks the few pixels of
// candidate t's bounding box inside the tile, tests them exactly as the pixel thread would (same expressions on the same
// operands) and appends t to the hit list of every pixel it covers (LDS counters); the pixel threads then insert only
// their own hits.  The K-best rule is a total order on (z, id), so the arrival order in the lists does not matter.  A
// pixel's first kHitList hits of a chunk go to its list, the others set the candidate's bit in the pixel's mask (s_more:
// 256 bits), which the pixel thread walks after its list.  Up to kWideCap candidates per chunk whose box covers more than
// kWideArea pixels are tested by every pixel thread instead.  (The first form had every pixel thread walk the
// candidates that reach its wave's four rows and test each one: the K-best insertion, ~50 instructions, ran for the whole
// wave whenever ANY of its lanes was hit -- with splats a few pixels wide that is nearly every candidate.)
// (Round 4, when a pixel with more hits than list entries tested ALL 256 candidates: 32 / 24 / 16-entry lists 316 / 333 /
// 429 us against 302 with 40; wide boxes from 24 / 48 / 96 / 192 pixels: 367 / 302 / 294 / 298 us.  Round 5 knock-outs at the
// scale of one rank's band of 8, SIREN surface: that overfull path was 43 of the kernel's 98 us -- a silhouette tile
// holds pixels with more than 40 hits in nearly every chunk, and each of them kept its whole wave for 256 tests.)
constexpr int kHitList = 32, kWideArea = 96, kWideCap = 32;

// KFULL: points_per_pixel == KMAX (4 / 8 / 16 / 32: the usual settings) -- K is then a compile-time constant and the
// per-slot `j < K` tests, the selection of the list's last live entry and their scalar branches fold away (a third of
// the instructions of an insertion).  (Seven workgroups per CU leave 72 vector registers; the runtime-K form needs one
// more and takes six -- a raster kernel must not spill, tests/test_abi.py.)
template <int KMAX, bool KFULL = false>
__global__ __launch_bounds__(256, KMAX <= 8 ? (KFULL ? 7 : 6) : 1) void k_raster(
    const float* __restrict__ pts, const float* __restrict__ ellipse,
    const float* __restrict__ cutoff, const float* __restrict__ radii,
    const int32_t* __restrict__ tile_order, const int4* __restrict__ items, const int32_t* __restrict__ item_count,
    float* __restrict__ scratch, const int32_t* __restrict__ tile_off,
    const int32_t* __restrict__ pairs, int64_t capacity, Frame F,
    int K_arg, float depth_thres, int32_t* __restrict__ idx_out, float* __restrict__ zbuf_out, float* __restrict__ q_out,
    float* __restrict__ occ_out, CompositeArgs ca) {
  const int K = KFULL ? KMAX : K_arg;
  __shared__ int s_hits[256];                                                // hits of the chunk per pixel
  __shared__ __attribute__((aligned(16))) unsigned char s_hit[256][kHitList];   // the first kHitList of them
  __shared__ unsigned s_more[8][256];                                        // the others: bit k % 32 of word [k / 32][pixel]
  // workgroups take the tiles of the band heaviest first (k_tile_order): a tile on the sphere's
  // silhouette holds 8x the mean number of candidates and would otherwise finish long after the rest
  // a work item = a tile, or -- for the tiles that hold many times the mean number of candidates (a
  // silhouette) -- one slice of its candidate list; the K-best lists of the slices are merged afterwards
  // (k_raster_merge), so the longest item is a slice, not the heaviest tile
  int tile, slice = 0, nslices = 1, slot = 0;
  if (items) {
    if ((int)blockIdx.x >= *item_count) return;
    const int4 it = items[blockIdx.x];
    tile = it.x; slice = it.y; nslices = it.z; slot = it.w;
  } else {
    tile = tile_order[blockIdx.x];
  }
  const int tx = tile % F.Tx, ty = (tile / F.Tx) % F.Ty, n = tile / (F.Tx * F.Ty);
  const int lx = threadIdx.x % TILE, ly = threadIdx.x / TILE;
  const int xi = tx * TILE + lx, yi = ty * TILE + ly;  // NDC pixel index
  const bool inside = xi < F.W && yi < F.H;
  const float xf = ndc_x(xi, F), yf = ndc_y(yi, F);
  // NDC y-range of the tile's four row bands.  Nothing reads them since the per-row candidate walk is gone; they stay
  // because dropping them changes this kernel's machine code (the compiler schedules their ndc_y work with yf's).
  float band_lo[4], band_hi[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    band_lo[w] = ndc_y(ty * TILE + 4 * w, F) - 1.0e-6f;
    band_hi[w] = ndc_y(ty * TILE + 4 * w + 3, F) + 1.0e-6f;
  }
  PixK<KMAX> best;
  best.init();
  float wz = FLT_MAX;
  int wi = 0x7fffffff;
  const int64_t off = tile_off[tile];
  int cnt = tile_off[tile + 1] - tile_off[tile];
  if (off + cnt > capacity) cnt = off < capacity ? (int)(capacity - off) : 0;  // overflow guard
  int c_begin = 0;
  if (nslices > 1) {                       // slice s of ns: chunk-aligned share of the list
    const int chunks = (cnt + 255) / 256;
    c_begin = (int)((int64_t)chunks * slice / nslices) * 256;
    cnt = min(cnt, (int)((int64_t)chunks * (slice + 1) / nslices) * 256);
  }
  // records of a chunk: {x, y, z, id} in LDS (the pixel threads read depth and id of their hits); {a, b, c, cutoff}
  // {rx, ry} stay in the registers of the thread that walks the candidate's box -- only the few wide candidates put
  // theirs in a small table for the pixel threads.  The next chunk's records are requested (into registers) while
  // this one is worked on.
  // ONE record buffer (a third barrier per chunk): 22.5 KB of LDS instead of 37 put seven workgroups on a CU
  // instead of four -- 387 -> 302 us; the kernel is bound by what the resident waves can overlap
  __shared__ float4 s_r0[256];
  __shared__ short s_wide[2][kWideCap];
  __shared__ float s_wrec[2][kWideCap][6];              // {a, b, c, cutoff, rx, ry}
  __shared__ int s_nw[2];
  float4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
  float2 r2 = {0.f, 0.f};
  auto fetch = [&](int c0) {
    if (c0 + (int)threadIdx.x < cnt) {
      const int p = pairs[off + c0 + threadIdx.x];
      r0 = make_float4(pts[(int64_t)p * 3], pts[(int64_t)p * 3 + 1], pts[(int64_t)p * 3 + 2], __int_as_float(p));
      r1 = make_float4(ellipse[(int64_t)p * 3], ellipse[(int64_t)p * 3 + 1], ellipse[(int64_t)p * 3 + 2], cutoff[p]);
      r2 = make_float2(radii[(int64_t)p * 2], radii[(int64_t)p * 2 + 1]);
    }
  };
  int par = 0;
  auto push_if_better = [&](const float4& c0v) {
    const float pz = c0v.z + 0.0f;                     // (-0 -> +0: push_masked orders depths by their bit patterns)
    const int id = __float_as_int(c0v.w);
    if (pz < wz || (pz == wz && id < wi)) {
      best.push_masked(pz, id, K);
      if (K == KMAX) { wz = best.z[KMAX - 1]; wi = best.id[KMAX - 1]; }
      else {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j == K - 1) { wz = best.z[j]; wi = best.id[j]; }
      }
    }
  };
  auto hit_push = [&](int k) { push_if_better(s_r0[k]); };                      // a listed hit: it passed the tests already
  // The inside test below and the one of the candidate walk are pixel_inside_point (splat_pixel.h) written out: the
  // call merges the two early exits into one branch and this kernel's machine code changes (tools/kernel_isa_diff.py).
  auto wide_push = [&](int i) {                                                  // entry i of the wide table, tested here
    const float4 c0v = s_r0[s_wide[par][i]];
    const float* wr = s_wrec[par][i];
    const float dx = xf - c0v.x, dy = yf - c0v.y;
    if (fabsf(dx) > wr[4] || fabsf(dy) > wr[5]) return;                          // rasterize_points.cu:92
    const float q = wr[0] * dx * dx + wr[1] * dx * dy + wr[2] * dy * dy;          // :94
    if (q > wr[3]) return;                                                       // :96
    push_if_better(c0v);
  };
  s_hits[threadIdx.x] = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) s_more[w][threadIdx.x] = 0u;
  if (threadIdx.x < 2) s_nw[threadIdx.x] = 0;
  fetch(c_begin);
  for (int c0 = c_begin; c0 < cnt; c0 += 256, par ^= 1) {
    const int m = min(256, cnt - c0);
    const float4 c0v = r0, c1v = r1;                    // this thread's candidate of the chunk
    const float2 c2v = r2;
    if ((int)threadIdx.x < m) s_r0[threadIdx.x] = r0;
    __syncthreads();                                    // records visible; the hit counters are zero
    fetch(c0 + 256);
    if ((int)threadIdx.x < m) {
      const int k = threadIdx.x;
      int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
      const bool any = pixel_range(c0v.x, c2v.x, F.W, F.ex, F.m, x0, x1) && pixel_range(c0v.y, c2v.y, F.H, F.ey, F.m, y0, y1);
      x0 = max(x0, tx * TILE); x1 = min(x1, tx * TILE + TILE - 1);
      y0 = max(y0, ty * TILE); y1 = min(y1, ty * TILE + TILE - 1);
      bool walk = any && x0 <= x1 && y0 <= y1;
      if (walk && (x1 - x0 + 1) * (y1 - y0 + 1) > kWideArea) {
        const int ws = atomicAdd(&s_nw[par], 1);
        if (ws < kWideCap) {                            // (a full table: the box is walked like the others)
          s_wide[par][ws] = (short)k;
          float* wr = s_wrec[par][ws];
          wr[0] = c1v.x; wr[1] = c1v.y; wr[2] = c1v.z; wr[3] = c1v.w; wr[4] = c2v.x; wr[5] = c2v.y;
          walk = false;
        }
      }
      if (walk) {
        for (int y = y0; y <= y1; ++y) {
          const float dy = ndc_y(y, F) - c0v.y;
          if (fabsf(dy) > c2v.y) continue;
          for (int x = x0; x <= x1; ++x) {
            const float dx = ndc_x(x, F) - c0v.x;
            if (fabsf(dx) > c2v.x) continue;
            const float q = c1v.x * dx * dx + c1v.y * dx * dy + c1v.z * dy * dy;
            if (q > c1v.w) continue;
            const int pl = (y - ty * TILE) * TILE + (x - tx * TILE);
            const int slot = atomicAdd(&s_hits[pl], 1);
            if (slot < kHitList) s_hit[pl][slot] = (unsigned char)k;
            else atomicOr(&s_more[k >> 5][pl], 1u << (k & 31));         // beyond the list: the pixel's bit mask
          }
        }
      }
    }
    __syncthreads();                                    // hit lists complete
    const int nh = s_hits[threadIdx.x];
    s_hits[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_nw[par ^ 1] = 0;
    if (inside) {
      const int nl = min(nh, kHitList);
      for (int i = 0; i < nl; ++i) hit_push(s_hit[threadIdx.x][i]);
      if (nh > kHitList) {
#pragma unroll 1
        for (int w = 0; w < 8; ++w) {
          unsigned mm = s_more[w][threadIdx.x];
          s_more[w][threadIdx.x] = 0u;
          while (mm) {
            const int b = __ffs((int)mm) - 1;
            mm &= mm - 1u;
            hit_push(w * 32 + b);
          }
        }
      }
      const int nw = min(s_nw[par], kWideCap);
      for (int i = 0; i < nw; ++i) wide_push(i);
    }
    __syncthreads();                                    // one record buffer: all reads done before the next chunk lands
  }
  // q of the K survivors (:94; the same expression on the same operands as the hit test): their records are
  // re-read once per tile instead of carrying q through every insertion
  if (inside) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < K && best.z[j] < FLT_MAX) {
        const int64_t p = best.id[j];
        const float dx = xf - pts[p * 3], dy = yf - pts[p * 3 + 1];
        best.q[j] = ellipse[p * 3] * dx * dx + ellipse[p * 3 + 1] * dx * dy + ellipse[p * 3 + 2] * dy * dy;
      }
    }
  }
  if (nslices > 1) {                       // partial result: the raw K-best of this slice, [z | q | id][k][pixel]
    float* sc = scratch + (int64_t)slot * 3 * KMAX * 256;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      sc[j * 256 + threadIdx.x] = best.z[j];
      sc[(KMAX + j) * 256 + threadIdx.x] = best.q[j];
      sc[(2 * KMAX + j) * 256 + threadIdx.x] = __int_as_float(best.id[j]);
    }
    return;
  }
  if (!inside) return;
  // output pixel is flipped in both axes (+X left, +Y up; rasterize_points.cu:577-580)
  const int yo = F.H - 1 - yi, xo = F.W - 1 - xi;
  const int64_t pix = ((int64_t)n * F.H + yo) * F.W + xo;
  // write_pixel_lists (splat_pixel.h) with the visible marks added.  Its text and not a call, here and in k_raster_merge: the
  // call changed the instruction schedule of both kernels (tools/kernel_isa_diff.py).
  const float z0 = best.z[0];
  const bool hit = z0 < FLT_MAX;
  occ_out[pix] = hit ? 1.0f : 0.0f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < K) {
      const bool ok = best.z[j] < FLT_MAX && !((best.z[j] - z0) > depth_thres);
      idx_out[pix * K + j] = ok ? best.id[j] : -1;
      zbuf_out[pix * K + j] = ok ? best.z[j] : -1.0f;
      q_out[pix * K + j] = ok ? best.q[j] : -1.0f;
      if (ok && ca.vis) ca.vis[best.id[j]] = 1;
    }
  }
  if (ca.scaler) composite_pixel<KMAX>(best, K, z0, depth_thres, hit, ca, pix);
}

// points_per_pixel above 32: the pixel's list is a DeepList (splat_pixel.h).  One workgroup per tile, every pixel thread
// tests every candidate of the tile; same (z, id) order, same outputs as k_raster.
__global__ __launch_bounds__(256) void k_raster_deep(
    const float* __restrict__ pts, const float* __restrict__ ellipse, const float* __restrict__ cutoff,
    const float* __restrict__ radii, const int32_t* __restrict__ tile_order, const int32_t* __restrict__ tile_off,
    const int32_t* __restrict__ pairs, int64_t capacity, Frame F, int K, float depth_thres,
    int32_t* __restrict__ idx_out, float* __restrict__ zbuf_out, float* __restrict__ q_out, float* __restrict__ occ_out,
    CompositeArgs ca) {
  __shared__ float s_px[256], s_py[256], s_pz[256], s_a[256], s_b[256], s_c[256], s_rx[256], s_ry[256], s_cut[256];
  __shared__ int s_id[256];
  const int tile = tile_order[blockIdx.x];
  const int tx = tile % F.Tx, ty = (tile / F.Tx) % F.Ty, n = tile / (F.Tx * F.Ty);
  const int lx = threadIdx.x % TILE, ly = threadIdx.x / TILE;
  const int xi = tx * TILE + lx, yi = ty * TILE + ly;
  const bool inside = xi < F.W && yi < F.H;
  const float xf = ndc_x(xi, F), yf = ndc_y(yi, F);
  const int yo = F.H - 1 - yi, xo = F.W - 1 - xi;
  const int64_t pix = ((int64_t)n * F.H + yo) * F.W + xo;
  DeepList best(idx_out, zbuf_out, q_out, pix, K);      // (its rows are only touched when inside)
  const int64_t off = tile_off[tile];
  int cnt = tile_off[tile + 1] - tile_off[tile];
  if (off + cnt > capacity) cnt = off < capacity ? (int)(capacity - off) : 0;
  for (int c0 = 0; c0 < cnt; c0 += 256) {
    const int m = min(256, cnt - c0);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const int p = pairs[off + c0 + threadIdx.x];
      s_px[threadIdx.x] = pts[(int64_t)p * 3]; s_py[threadIdx.x] = pts[(int64_t)p * 3 + 1]; s_pz[threadIdx.x] = pts[(int64_t)p * 3 + 2];
      s_a[threadIdx.x] = ellipse[(int64_t)p * 3]; s_b[threadIdx.x] = ellipse[(int64_t)p * 3 + 1]; s_c[threadIdx.x] = ellipse[(int64_t)p * 3 + 2];
      s_rx[threadIdx.x] = radii[(int64_t)p * 2]; s_ry[threadIdx.x] = radii[(int64_t)p * 2 + 1];
      s_cut[threadIdx.x] = cutoff[p]; s_id[threadIdx.x] = p;
    }
    __syncthreads();
    if (!inside) continue;
    for (int k = 0; k < m; ++k) {
      float q;
      if (pixel_inside_point(xf - s_px[k], yf - s_py[k], s_a[k], s_b[k], s_c[k], s_rx[k], s_ry[k], s_cut[k], q))
        best.push(s_pz[k], s_id[k], q);
    }
  }
  if (!inside) return;
  // the image first: it reads the list's rows before the cut overwrites the dropped ones
  if (ca.scaler) composite_pixel<0>(best, best.have, best.front(), depth_thres, best.have > 0, ca, pix);
  best.finish(depth_thres, occ_out, pix, ca.vis);
}

// Tiles of the band [ty_begin, ty_begin+ty_rows) of every cloud, heaviest first (64 buckets of the
// candidate count; the order inside a bucket is arbitrary -- it only affects scheduling).
__global__ __launch_bounds__(1024) void k_tile_order(const int32_t* __restrict__ tile_off, Frame F, int ty_begin,
                                                     int ty_rows, int n_clouds, int32_t* __restrict__ order) {
  const int T = F.Tx, TY = F.Ty;
  __shared__ int hist[64], base[64];
  const int tiles = n_clouds * T * ty_rows;
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  __syncthreads();
  auto tile_of = [&](int i) { return ((i / (T * ty_rows)) * TY + ty_begin + (i / T) % ty_rows) * T + i % T; };
  auto bucket_of = [&](int tile) {
    const int c = tile_off[tile + 1] - tile_off[tile];
    return min(c >> 6, 63);
  };
  for (int i = threadIdx.x; i < tiles; i += blockDim.x) atomicAdd(&hist[bucket_of(tile_of(i))], 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int b = 63; b >= 0; --b) { base[b] = run; run += hist[b]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < tiles; i += blockDim.x) {
    const int tile = tile_of(i);
    order[atomicAdd(&base[bucket_of(tile)], 1)] = tile;
  }
}

// Work items of a band (see k_raster): tiles with more than 1.5 slices of candidates are cut into slices
// (<= kSlice candidates each) as long as the scratch slots last; slices first, then the whole tiles heaviest
// first.  heavy[h] = (tile, first scratch slot, slices).  counters: [0] items, [1] heavy tiles.
// (kTargetItems, cfg-3a cycle, 1.4 M candidates over 4096 tiles: slices of 1024 / 512 / 256 candidates -- targets 2048 / 3072..5120 /
// >= 6144 -- raster + merge 288 + 29 / 224 + 37 / 206 + 63 us)
constexpr int kSlice = 1024, kTargetItems = 4096;
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// one workgroup of any size that is a multiple of 64
__device__ void tile_items_body(const int32_t* __restrict__ tile_off, Frame F, int ty_begin,
                                int ty_rows, int n_clouds, int max_slots, int target_items,
                                int4* __restrict__ items, int4* __restrict__ heavy,
                                int32_t* __restrict__ counters) {
  __shared__ int hist[64], base[64];
  __shared__ int s_slots, s_heavy, s_slice;
  const int T = F.Tx, TY = F.Ty;
  const int tiles = n_clouds * T * ty_rows;
  auto tile_of = [&](int i) { return ((i / (T * ty_rows)) * TY + ty_begin + (i / T) % ty_rows) * T + i % T; };
  auto count_of = [&](int tile) { return tile_off[tile + 1] - tile_off[tile]; };
  // slice size: total candidates / kTargetItems (so that a small band still yields enough work items to
  // fill the chip), within [256, kSlice], doubled until the slices of all cut tiles fit the scratch slots.
  // A thread's first four tiles (all of them up to 4096 tiles) are read once and kept in registers: every
  // pass below would otherwise start with the same global-memory latency.
  int cc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = threadIdx.x + k * (int)blockDim.x;
    cc[k] = i < tiles ? count_of(tile_of(i)) : 0;
  }
  // visit(f): f(i, tile, count) for every tile of this thread
  auto visit = [&](auto&& f) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = threadIdx.x + k * (int)blockDim.x;
      if (i < tiles) f(i, tile_of(i), cc[k]);
    }
    for (int i = threadIdx.x + 4 * (int)blockDim.x; i < tiles; i += blockDim.x) f(i, tile_of(i), count_of(tile_of(i)));
  };
  if (threadIdx.x == 0) s_slots = 0;
  __syncthreads();
  {
    int mine = 0;
    visit([&](int, int, int c) { mine += c; });
    mine = wave_sum_i(mine);                              // (a thousand same-address LDS atomics are ~4 us of this single-workgroup kernel)
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_slots, mine);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int sl0 = (s_slots / target_items + 255) / 256 * 256;
    s_slice = sl0 < 256 ? 256 : (sl0 > kSlice ? kSlice : sl0);
  }
  __syncthreads();
  for (int round = 0; round < 16; ++round) {
    if (threadIdx.x == 0) s_slots = 0;
    __syncthreads();
    const int sl = s_slice;
    int mine = 0;
    visit([&](int, int, int c) { if (2 * c > 3 * sl) mine += (c + sl - 1) / sl; });
    mine = wave_sum_i(mine);                              // (a thousand same-address LDS atomics are ~4 us of this single-workgroup kernel)
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_slots, mine);
    __syncthreads();
    const bool fits = s_slots <= max_slots;
    __syncthreads();
    if (fits) break;
    if (threadIdx.x == 0) s_slice = sl * 2;
    __syncthreads();
  }
  const int sl = s_slice;
  auto slices_of = [&](int c) { return (2 * c > 3 * sl && max_slots > 0) ? (c + sl - 1) / sl : 1; };
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) { s_slots = 0; s_heavy = 0; }
  __syncthreads();
  auto bucket_of = [&](int c) { return min(c >> 6, 63); };
  visit([&](int, int tile, int c) {
    const int ns = slices_of(c);
    if (ns > 1) {
      const int b0 = atomicAdd(&s_slots, ns);
      heavy[atomicAdd(&s_heavy, 1)] = make_int4(tile, b0, ns, 0);
      for (int k = 0; k < ns; ++k) items[b0 + k] = make_int4(tile, k, ns, b0 + k);
    } else {
      atomicAdd(&hist[bucket_of(c)], 1);
    }
  });
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = s_slots;
    for (int b = 63; b >= 0; --b) { base[b] = run; run += hist[b]; }
    counters[0] = run;
    counters[1] = s_heavy;
  }
  __syncthreads();
  visit([&](int, int tile, int c) {
    if (slices_of(c) == 1) items[atomicAdd(&base[bucket_of(c)], 1)] = make_int4(tile, 0, 1, 0);
  });
}
__global__ __launch_bounds__(1024) void k_tile_items(const int32_t* __restrict__ tile_off, Frame F, int ty_begin,
                                                     int ty_rows, int n_clouds, int max_slots, int target_items,
                                                     int4* __restrict__ items, int4* __restrict__ heavy,
                                                     int32_t* __restrict__ counters) {
  tile_items_body(tile_off, F, ty_begin, ty_rows, n_clouds, max_slots, target_items, items, heavy, counters);
}

// K-best of a heavy tile's pixels from the K-best lists of its slices (same (z, idx) order: the result
// does not depend on how the list was cut), then the depth-merging cut and the outputs of k_raster.
template <int KMAX, bool KFULL = false>
__global__ __launch_bounds__(256) void k_raster_merge(const int4* __restrict__ heavy, const int32_t* __restrict__ counters,
                                                      const float* __restrict__ scratch, Frame F, int K_arg,
                                                      float depth_thres, int32_t* __restrict__ idx_out,
                                                      float* __restrict__ zbuf_out, float* __restrict__ q_out,
                                                      float* __restrict__ occ_out, CompositeArgs ca) {
  const int K = KFULL ? KMAX : K_arg;
  const int nh = counters[1];
  for (int hI = blockIdx.x; hI < nh; hI += gridDim.x) {
    const int4 hv = heavy[hI];
    const int tile = hv.x;
    const int tx = tile % F.Tx, ty = (tile / F.Tx) % F.Ty, n = tile / (F.Tx * F.Ty);
    const int lx = threadIdx.x % TILE, ly = threadIdx.x / TILE;
    const int xi = tx * TILE + lx, yi = ty * TILE + ly;
    PixK<KMAX> best;
    best.init();
    for (int sI = 0; sI < hv.z; ++sI) {
      // a slice's list is requested whole before any of it is used (the id / q loads sat behind the depth test);
      // the first slice's list IS the K-best so far
      const float* sc = scratch + (int64_t)(hv.y + sI) * 3 * KMAX * 256;
      float zz[KMAX], qq[KMAX];
      int ii[KMAX];
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        zz[j] = sc[j * 256 + threadIdx.x];
        qq[j] = sc[(KMAX + j) * 256 + threadIdx.x];
        ii[j] = __float_as_int(sc[(2 * KMAX + j) * 256 + threadIdx.x]);
      }
      if (sI == 0) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { best.z[j] = zz[j]; best.q[j] = qq[j]; best.id[j] = ii[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
          if (j < K && zz[j] < FLT_MAX) best.template push_masked<true>(zz[j], ii[j], K, qq[j]);   // (slice lists hold depths >= +0)
      }
    }
    if (xi >= F.W || yi >= F.H) continue;
    const int yo = F.H - 1 - yi, xo = F.W - 1 - xi;
    const int64_t pix = ((int64_t)n * F.H + yo) * F.W + xo;
    const float z0 = best.z[0];                            // write_pixel_lists' text (see k_raster)
    const bool hit = z0 < FLT_MAX;
    occ_out[pix] = hit ? 1.0f : 0.0f;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < K) {
        const bool ok = best.z[j] < FLT_MAX && !((best.z[j] - z0) > depth_thres);
        idx_out[pix * K + j] = ok ? best.id[j] : -1;
        zbuf_out[pix * K + j] = ok ? best.z[j] : -1.0f;
        q_out[pix * K + j] = ok ? best.q[j] : -1.0f;
        if (ok && ca.vis) ca.vis[best.id[j]] = 1;
      }
    }
    if (ca.scaler) composite_pixel<KMAX>(best, K, z0, depth_thres, hit, ca, pix);
  }
}

}  // namespace

// ===========================================================================
extern "C" int iso_splat_tiles_per_side(int image_size) { return (image_size + TILE - 1) / TILE; }

extern "C" int iso_splat_bin_count(const float* points, const float* radii,
                                   const int64_t* first_idx, const int64_t* num_pts, int n_clouds,
                                   int64_t max_pts, int image_size, int image_width, int tile_row_begin,
                                   int tile_row_end, int32_t* tile_cnt, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && max_pts >= 0 && image_size > 0, ISO_ERR_INVALID, "iso_splat_bin_count: bad sizes");
  if (n_clouds == 0 || max_pts == 0) return ISO_OK;
  ISO_REQUIRE(points && radii && first_idx && num_pts && tile_cnt, ISO_ERR_INVALID,
              "iso_splat_bin_count: null pointer");
  const Frame F = make_frame(image_size, image_width > 0 ? image_width : image_size);
  ISO_REQUIRE(tile_row_begin >= 0 && tile_row_begin <= tile_row_end && tile_row_end <= F.Ty,
              ISO_ERR_INVALID, "iso_splat_bin_count: bad tile row band");
  launch_bin<false>(points, radii, first_idx, num_pts, n_clouds, max_pts, F, tile_row_begin,
                    tile_row_end, tile_cnt, nullptr, nullptr, 0, nullptr, (hipStream_t)stream);
  ISO_CHECK_LAUNCH("iso_splat_bin_count");
  return ISO_OK;
}

namespace {
// exclusive scan of the n tile counters by ONE workgroup (n = views x tiles + 1: a few thousand entries -- three
// launches of a general multi-block scan for them were three launch latencies); the counters are cleared as they
// are read (the next binning pass finds them zero) and the fill cursors start at zero
__global__ __launch_bounds__(1024) void k_tile_offsets(int32_t* __restrict__ cnt, int32_t* __restrict__ off,
                                                       int32_t* __restrict__ cursor, int64_t n) {
  __shared__ int s_w[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int carry = 0;
  for (int64_t c0 = 0; c0 < n; c0 += 4096) {
    const int64_t i0 = c0 + (int64_t)threadIdx.x * 4;
    int v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0;
      if (i0 + k < n) { v[k] = cnt[i0 + k]; cnt[i0 + k] = 0; cursor[i0 + k] = 0; }
      sum += v[k];
    }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int sv = s_w[k]; if (k < w) base += sv; tot += sv; }
    int ex = carry + base + inc - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < n) off[i0 + k] = ex;
      ex += v[k];
    }
    carry += tot;
    __syncthreads();
  }
}
}  // namespace

extern "C" int iso_splat_tile_offsets(int32_t* tile_cnt, int32_t* tile_off, int32_t* tile_cursor, int64_t n, void* stream) {
  ISO_REQUIRE(n >= 0 && (n == 0 || (tile_cnt && tile_off && tile_cursor)), ISO_ERR_INVALID, "iso_splat_tile_offsets: bad arguments");
  if (n == 0) return ISO_OK;
  hipLaunchKernelGGL(k_tile_offsets, dim3(1), dim3(1024), 0, (hipStream_t)stream, tile_cnt, tile_off, tile_cursor, n);
  ISO_CHECK_LAUNCH("iso_splat_tile_offsets");
  return ISO_OK;
}

extern "C" int64_t iso_splat_forward_workspace_bytes(int64_t n_tiles, int points_per_pixel) {
  const int K = points_per_pixel;
  const int KM = K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 16 ? 16 : 32));
  if (n_tiles < 0) n_tiles = 0;
  int64_t slots = n_tiles / 2 + 256;               // room to cut every other tile once; k_tile_items adapts the slice size
  if (slots < 2048) slots = 2048;                  // a small band is cut finer (enough work items to fill the chip)
  if (slots > 8192) slots = 8192;
  return 64 + 32 * n_tiles + slots * (16 + (int64_t)3 * KM * 256 * 4);
}

static int splat_forward_impl(CompositeArgs ca, const float* points, const float* ellipse, const float* cutoff,
                                 const float* radii, const int64_t* first_idx,
                                 const int64_t* num_pts, int n_clouds, int64_t max_pts,
                                 float depth_merging_thres, int image_size, int image_width, int points_per_pixel,
                                 int tile_row_begin, int tile_row_end, int32_t* tile_cursor,
                                 const int32_t* tile_off, int32_t* pairs,
                                 int64_t pair_capacity, int32_t* overflow_flag, int32_t* idx_out,
                                 float* zbuf_out, float* qvalue_out, float* occ_out, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(points_per_pixel >= 1 && points_per_pixel <= 150, ISO_ERR_UNSUPPORTED,
              "iso_splat_forward: points_per_pixel must be in [1,150] (rasterization_utils.cuh:18), got %d", points_per_pixel);
  ISO_REQUIRE(n_clouds >= 0 && max_pts >= 0 && image_size > 0, ISO_ERR_INVALID, "iso_splat_forward: bad sizes");
  if (n_clouds == 0) return ISO_OK;
  ISO_REQUIRE(first_idx && num_pts && tile_cursor && tile_off && overflow_flag && idx_out &&
                  zbuf_out && qvalue_out && occ_out && (pairs || pair_capacity == 0),
              ISO_ERR_INVALID, "iso_splat_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Frame F = make_frame(image_size, image_width > 0 ? image_width : image_size);
  const int T = F.Tx;
  ISO_REQUIRE(tile_row_begin >= 0 && tile_row_begin <= tile_row_end && tile_row_end <= F.Ty,
              ISO_ERR_INVALID, "iso_splat_forward: bad tile row band");
  if (tile_row_begin == tile_row_end) return ISO_OK;
  const int ty_rows = tile_row_end - tile_row_begin;
  const int tiles = n_clouds * T * ty_rows;
  const int K = points_per_pixel;
  const int KM = K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 16 ? 16 : 32));
  // workspace (optional): work items with the heavy tiles cut into slices
  //   [counters 64 B][items int4 (tiles + slots)][heavy int4 (tiles)][scratch slots * 3 * KM * 256 floats]
  int max_slots = 0;
  int4* items = nullptr; int4* heavy = nullptr; int32_t* counters = nullptr; float* scratch = nullptr;
  if (workspace && tiles > 0 && K <= 32) {
    const int64_t per_slot = 16 + (int64_t)3 * KM * 256 * 4;
    const int64_t fixed = 64 + (int64_t)32 * tiles;
    int64_t slots = workspace_bytes > fixed ? (workspace_bytes - fixed) / per_slot : 0;
    if (slots > 65536) slots = 65536;
    max_slots = (int)slots;
    counters = (int32_t*)workspace;
    items = (int4*)((char*)workspace + 64);
    heavy = items + tiles + max_slots;
    scratch = (float*)(heavy + tiles);
  }
  bool items_done = false;
  if (max_pts > 0) {
    ISO_REQUIRE(points && ellipse && cutoff && radii, ISO_ERR_INVALID, "iso_splat_forward: null pointer");
    // the fill launch also makes the raster's work items (one more workgroup: they only need the offsets)
    items_done = launch_bin<true>(points, radii, first_idx, num_pts, n_clouds, max_pts, F, tile_row_begin,
                                  tile_row_end, tile_cursor, tile_off, pairs, pair_capacity, overflow_flag, s,
                                  TileItemsJob{ty_rows, n_clouds, max_slots, kTargetItems, items, heavy, counters});
  }
  if (K > 32) {                               // lists too deep for registers: one workgroup per tile, lists in the outputs
    hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, s, tile_off, F, tile_row_begin, ty_rows, n_clouds, tile_cursor);
    hipLaunchKernelGGL(k_raster_deep, dim3(tiles), dim3(256), 0, s, points, ellipse, cutoff, radii, tile_cursor, tile_off, pairs,
                       pair_capacity, F, K, depth_merging_thres, idx_out, zbuf_out, qvalue_out, occ_out, ca);
    ISO_CHECK_LAUNCH("iso_splat_forward");
    return ISO_OK;
  }
  if (items) {
    if (!items_done)
      hipLaunchKernelGGL(k_tile_items, dim3(1), dim3(1024), 0, s, tile_off, F, tile_row_begin, ty_rows, n_clouds, max_slots,
                         kTargetItems, items, heavy, counters);
  } else {
    // the fill cursors are dead now: their array takes the heaviest-first tile order
    hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, s, tile_off, F, tile_row_begin, ty_rows, n_clouds,
                       tile_cursor);
  }
#define ISO_LAUNCH_R(KM_)                                                                            \
  if (K == KM_)                                                                                      \
    hipLaunchKernelGGL((k_raster<KM_, true>), dim3(tiles + max_slots), dim3(256), 0, s, points, ellipse, cutoff, radii, \
                       tile_cursor, items, counters, scratch, tile_off, pairs, pair_capacity, F,                \
                       K, depth_merging_thres, idx_out, zbuf_out, qvalue_out, occ_out, ca);             \
  else                                                                                               \
    hipLaunchKernelGGL((k_raster<KM_>), dim3(tiles + max_slots), dim3(256), 0, s, points, ellipse, cutoff, radii, \
                       tile_cursor, items, counters, scratch, tile_off, pairs, pair_capacity, F,                \
                       K, depth_merging_thres, idx_out, zbuf_out, qvalue_out, occ_out, ca);             \
  if (items && K == KM_)                                                                              \
    hipLaunchKernelGGL((k_raster_merge<KM_, true>), dim3(tiles < 1024 ? tiles : 1024), dim3(256), 0, s, heavy, counters, scratch, \
                       F, K, depth_merging_thres, idx_out, zbuf_out, qvalue_out, occ_out, ca);              \
  else if (items)                                                                                     \
    hipLaunchKernelGGL(k_raster_merge<KM_>, dim3(tiles < 1024 ? tiles : 1024), dim3(256), 0, s, heavy, counters, scratch, \
                       F, K, depth_merging_thres, idx_out, zbuf_out, qvalue_out, occ_out, ca)
  if (K <= 4) { ISO_LAUNCH_R(4); }
  else if (K <= 8) { ISO_LAUNCH_R(8); }
  else if (K <= 16) { ISO_LAUNCH_R(16); }
  else { ISO_LAUNCH_R(32); }
#undef ISO_LAUNCH_R
  ISO_CHECK_LAUNCH("iso_splat_forward");
  return ISO_OK;
}

extern "C" int iso_splat_forward(const float* points, const float* ellipse, const float* cutoff,
                                 const float* radii, const int64_t* first_idx,
                                 const int64_t* num_pts, int n_clouds, int64_t max_pts,
                                 float depth_merging_thres, int image_size, int image_width, int points_per_pixel,
                                 int tile_row_begin, int tile_row_end, int32_t* tile_cursor,
                                 const int32_t* tile_off, int32_t* pairs,
                                 int64_t pair_capacity, int32_t* overflow_flag, int32_t* idx_out,
                                 float* zbuf_out, float* qvalue_out, float* occ_out, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  CompositeArgs ca{nullptr, nullptr, nullptr, 0, 0, 0.f, nullptr};
  return splat_forward_impl(ca, points, ellipse, cutoff, radii, first_idx, num_pts, n_clouds, max_pts, depth_merging_thres,
                            image_size, image_width, points_per_pixel, tile_row_begin, tile_row_end, tile_cursor, tile_off, pairs,
                            pair_capacity, overflow_flag, idx_out, zbuf_out, qvalue_out, occ_out, workspace,
                            workspace_bytes, stream);
}

// iso_splat_forward + iso_splat_composite in one pass: the pixels' images are composited from the K-best
// lists while they are still in registers (same arithmetic and order as iso_splat_composite).
extern "C" int iso_splat_render(const float* points, const float* ellipse, const float* cutoff,
                                const float* radii, const int64_t* first_idx,
                                const int64_t* num_pts, int n_clouds, int64_t max_pts,
                                float depth_merging_thres, int image_size, int image_width, int points_per_pixel,
                                int tile_row_begin, int tile_row_end, int32_t* tile_cursor,
                                const int32_t* tile_off, int32_t* pairs,
                                int64_t pair_capacity, int32_t* overflow_flag, int32_t* idx_out,
                                float* zbuf_out, float* qvalue_out, float* occ_out, void* workspace,
                                int64_t workspace_bytes, const float* scaler, const float* features, int channels,
                                int norm_weighted, float eps, float* image_out, void* stream) {
  return iso_splat_render_visible(points, ellipse, cutoff, radii, first_idx, num_pts, n_clouds, max_pts, depth_merging_thres,
                                  image_size, image_width, points_per_pixel, tile_row_begin, tile_row_end, tile_cursor, tile_off,
                                  pairs, pair_capacity, overflow_flag, idx_out, zbuf_out, qvalue_out, occ_out, workspace,
                                  workspace_bytes, scaler, features, channels, norm_weighted, eps, image_out, nullptr, stream);
}

// ... and the visible flags of the backward pass (iso_splat_mark_visible) while the lists are written: visible_out (P,)
// uint8, ZERO on entry over the rows of the clouds (the front end clears them), 1 afterwards for every point that a
// pixel's list holds.
extern "C" int iso_splat_render_visible(const float* points, const float* ellipse, const float* cutoff,
                                        const float* radii, const int64_t* first_idx,
                                        const int64_t* num_pts, int n_clouds, int64_t max_pts,
                                        float depth_merging_thres, int image_size, int image_width, int points_per_pixel,
                                        int tile_row_begin, int tile_row_end, int32_t* tile_cursor,
                                        const int32_t* tile_off, int32_t* pairs,
                                        int64_t pair_capacity, int32_t* overflow_flag, int32_t* idx_out,
                                        float* zbuf_out, float* qvalue_out, float* occ_out, void* workspace,
                                        int64_t workspace_bytes, const float* scaler, const float* features, int channels,
                                        int norm_weighted, float eps, float* image_out, uint8_t* visible_out, void* stream) {
  ISO_REQUIRE(channels >= 0 && channels <= 8, ISO_ERR_UNSUPPORTED, "iso_splat_render: channels must be <= 8");
  ISO_REQUIRE(scaler && image_out && (features || channels == 0), ISO_ERR_INVALID, "iso_splat_render: null pointer");
  CompositeArgs ca{scaler, features, image_out, channels, norm_weighted, eps, visible_out};
  return splat_forward_impl(ca, points, ellipse, cutoff, radii, first_idx, num_pts, n_clouds, max_pts, depth_merging_thres,
                            image_size, image_width, points_per_pixel, tile_row_begin, tile_row_end, tile_cursor, tile_off, pairs,
                            pair_capacity, overflow_flag, idx_out, zbuf_out, qvalue_out, occ_out, workspace,
                            workspace_bytes, stream);
}
