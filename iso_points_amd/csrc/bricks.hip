// Brick grid (bricks.h), the build: the workspace and its carve, the header from a bounding box, and count -> offsets
// (+ work list) -> scatter of a cloud's records into brick order, with the imported halo records of N ranks and the
// chunk scan of the splat front end riding in its launches.  What searches the grid lives in files of its own:
//   bricks_stage.h      staging of a brick into LDS and the window walks, shared by the two fused kernels
//   bricks_walk.h       the ring walk of their tail kernels
//   bricks_resample.hip the fused resample step (FRNN K+1 query + tangent-plane repulsion)
//   bricks_h.hip        the fused per-view splat bandwidth h
//   bricks_halo.hip     the N-rank halo exchange
//
// Reference semantics
//   neighbour tree  : UniformProjection._create_tree, DSS/models/levelset_sampling.py:110-140
//                     (bbox of the cloud, r = sqrt(diag/P) * knn_k: bricks_header in bricks.h)
#include "bricks.h"
#include "follow.h"      // front_tile_table: where the chunk scan's tile counts lie

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
constexpr int kScan1MaxWords = 2048;        // = kScan1Max (k_brick_offsets1): chunk totals the one-launch scan keeps zeroed (BrickWs::scan1)
BrickWs bricks_carve(void* ws, int64_t n_max) {
  BrickWs w;
  if (n_max < 1) n_max = 1;
  w.nb_cap = bricks_nb_cap(n_max);
  w.G = BK_CPB * (int64_t)w.nb_cap * w.nb_cap * w.nb_cap + 1;   // BK_CPB counters per brick (bricks.h)
  auto al = [](int64_t b) { return (b + 255) / 256 * 256; };
  char* p = (char*)ws;
  int64_t o = 0;
  w.hdr = (BrickHdr*)(p + o); o += al(sizeof(BrickHdr));
  w.counters = (int32_t*)(p + o); o += al(4 * kCounterInts);
  w.scan1 = (unsigned*)(p + o); o += al(4 * kScan1MaxWords);          // fixed offset: independent of n_max
  w.cnt = (int32_t*)(p + o); o += al(4 * w.G);
  w.off = (int32_t*)(p + o); o += al(4 * w.G);
  w.slot = (int32_t*)(p + o); o += al(4 * n_max);
  w.rec0 = (float4*)(p + o); o += al(16 * n_max);
  w.rec1 = (float4*)(p + o); o += al(16 * n_max);
  w.list = (int32_t*)(p + o); o += al(4 * (w.G < n_max ? w.G : n_max));
  w.tail = (int32_t*)(p + o); o += al(4 * 8 * n_max);
  w.scan_ws_bytes = iso_prefix_sum_workspace_bytes(w.G, 1) + 4 * (kScan1MaxWords + (w.G + 1023) / 1024);   // (sums of the two-launch scan)
  w.scan_ws = (void*)(p + o); o += al(w.scan_ws_bytes);
  w.bytes = o;
  return w;
}

namespace {

// ---- header ------------------------------------------------------------------------------------
// bbox: [min xyz, 0, max xyz, 0] (iso_points_bbox layout; for N ranks the caller reduces it first)
__global__ void k_bricks_params(const float* __restrict__ bbox, int n_boxes, BrickParams q, BrickHdr* __restrict__ h,
                                int32_t* __restrict__ counters) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float mn[3], mx[3];
  for (int a = 0; a < 3; ++a) {                     // the union of the n_boxes boxes (N ranks: every rank's local box)
    float lo = bbox[a], hi = bbox[4 + a];
    for (int k = 1; k < n_boxes; ++k) { lo = fminf(lo, bbox[k * 8 + a]); hi = fmaxf(hi, bbox[k * 8 + 4 + a]); }
    mn[a] = lo; mx[a] = hi;
  }
  bricks_store_header(bricks_header(mn, mx, q), h, counters);
}

// Bounding box of a packed (n,3) cloud into the workspace's PENDING BOX (bricks.h): flat float index (consecutive lanes
// read consecutive dwords; the grid stride is a multiple of 3 floats, so a thread stays on one axis and keeps four loads
// in flight), registers -> wave shuffles -> LDS -> six atomics per workgroup on one of kBoxCopies copies.  The header is
// made from it by the count pass that follows.
__global__ __launch_bounds__(256) void k_brick_bbox(const float* __restrict__ p, int64_t n, int32_t* __restrict__ counters) {
  __shared__ float s_box[4][6];
  const int64_t nfl = n * 3;
  const int64_t stride = (int64_t)gridDim.x * 256;            // a multiple of 3 (launcher)
  const int64_t i_first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float lo = FLT_MAX, hi = -FLT_MAX;
  int64_t i = i_first;
  for (; i + 3 * stride < nfl; i += 4 * stride) {
    const float v0 = p[i], v1 = p[i + stride], v2 = p[i + 2 * stride], v3 = p[i + 3 * stride];
    lo = fminf(fminf(lo, v0), fminf(v1, fminf(v2, v3)));
    hi = fmaxf(fmaxf(hi, v0), fmaxf(v1, fmaxf(v2, v3)));
  }
  for (; i < nfl; i += stride) { const float v = p[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
  const int ax = (int)(i_first % 3);
  BkBox box;
#pragma unroll
  for (int c = 0; c < 3; ++c) { box.lo[c] = ax == c ? lo : FLT_MAX; box.hi[c] = ax == c ? hi : -FLT_MAX; }
  box.commit(counters, s_box);
}

// the pending box as 8 floats (iso_points_bbox layout): what N ranks all-gather before iso_bricks_params; cleared
__global__ __launch_bounds__(256) void k_brick_box_take(int32_t* __restrict__ counters, float* __restrict__ box_out) {
  __shared__ unsigned s_red[8];
  float mn[3], mx[3];
  bk_box_read(counters, s_red, mn, mx);
  __syncthreads();
  bk_box_clear(counters);
  if (threadIdx.x == 0) {
    for (int c = 0; c < 3; ++c) { box_out[c] = mn[c]; box_out[4 + c] = mx[c]; }
    box_out[3] = 0.f; box_out[7] = 0.f;
  }
}

// zero the whole table once (iso_bricks_workspace_init); afterwards the offsets pass leaves it zeroed
__global__ void k_bricks_init(int32_t* __restrict__ counters, int32_t* __restrict__ cnt, int64_t G, unsigned* __restrict__ scan_ws) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 < kScan1MaxWords) scan_ws[i0] = 0u;
  for (int64_t i = i0; i < G; i += (int64_t)gridDim.x * blockDim.x) cnt[i] = 0;
  for (int64_t i = i0; i < kCounterInts; i += (int64_t)gridDim.x * blockDim.x) counters[i] = i == kMagicAt ? kBrickMagic : 0;
}

// F.normalize(n, dim=-1): n / max(|n|, 1e-12) (levelset_sampling.py:258), stored in rec1 in place of the raw normal
__device__ __forceinline__ void bk_unit_normal(float& ux, float& uy, float& uz) {
  float un = sqrtf((ux * ux + uy * uy) + uz * uz);
  un = un > 1e-12f ? un : 1e-12f;
  ux = ux / un; uy = uy / un; uz = uz / un;
}

// counter of a point: BK_CPB * brick + sub-brick (bricks.h)
__device__ __forceinline__ int counter_of(const BrickHdr& h, float x, float y, float z) {
  const int fx = bk_fine(x, h.mn[0], h.inv_f, h.nf[0]);
  const int fy = bk_fine(y, h.mn[1], h.inv_f, h.nf[1]);
  const int fz = bk_fine(z, h.mn[2], h.inv_f, h.nf[2]);
  const int brick = ((fx >> 2) * h.nb[1] + (fy >> 2)) * h.nb[2] + (fz >> 2);
  return BK_CPB * brick + ((((fx >> 1) & 1) * 2 + ((fy >> 1) & 1)) * 2 + ((fz >> 1) & 1));
}

// Arrival slot of a record inside its brick (own points: packed (n,3) f32; imported halo records: float4).  The records
// of brick b are [off[BK_CPB b], off[BK_CPB (b + 1)]) whatever the order inside.  A workgroup first counts its 1024
// records per brick in an LDS hash table and then reserves each brick's range with ONE returning global atomic (a
// record order with any spatial coherence -- the cycle's clouds run along a z-order curve -- puts many of a round's
// records in the same brick; one returning atomic per record was the whole cost of this pass).  All records of a
// workgroup that fall into one counter (sub-brick) get consecutive ranks; slot = rank; a record that finds no table
// entry within kCntProbe probes takes its rank from global memory directly.
constexpr int kCntTab = 2048, kCntProbe = 16;

// one round of 1024 records of a workgroup: pos(i, x, y, z) fetches record i, its slot goes to slot_out[i]
template <class Pos>
__device__ __forceinline__ void brick_count_round(const BrickHdr& h, int64_t base, int64_t n, int32_t* __restrict__ cnt,
                                                  int32_t* __restrict__ slot_out, int* t_key, int* t_cnt, Pos&& pos) {
  for (int j = threadIdx.x; j < kCntTab; j += 256) { t_key[j] = -1; t_cnt[j] = 0; }
  __syncthreads();
  int e[4], rk[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    e[k] = -1; rk[k] = 0;
    if (i < n) {
      float x, y, z;
      pos(i, k, x, y, z);
      const int key = counter_of(h, x, y, z);
      unsigned at = ((unsigned)key * 2654435761u) >> 21;          // 11 bits
      bool found = false;
      for (int t = 0; t < kCntProbe && !found; ++t) {
        const int prev = atomicCAS(&t_key[at], -1, key);
        if (prev == -1 || prev == key) found = true;
        else at = (at + 1) & (kCntTab - 1);
      }
      if (found) { e[k] = (int)at; rk[k] = atomicAdd(&t_cnt[at], 1); }
      else rk[k] = atomicAdd(&cnt[key], 1);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kCntTab; j += 256) {
    const int c = t_cnt[j];
    if (c > 0) t_cnt[j] = atomicAdd(&cnt[t_key[j]], c);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < n) slot_out[i] = (e[k] >= 0 ? t_cnt[e[k]] : 0) + rk[k];       // rank inside the point's counter (sub-brick)
  }
  __syncthreads();
}

// pending != 0: the header is not written yet -- it is made HERE from the workspace's pending box, by every workgroup
// for itself (sixteen 32-byte words from L2 + a few dozen scalar operations; a launch of its own cost 5 us, a "last workgroup
// writes it" tail in the pass that took the box 7 us); the last workgroup also stores it for the launches that follow and
// retires the counters of the previous grid.
// job != null: workgroup 0 of the grid does not count -- it runs the chunk scan of the splat front end beside
// the others (ChunkScanJob, below).
struct ChunkScanJob {
  const int32_t* tile_cnt;   // (n_views, n_tiles) renderable points per 256-point tile (follow.h) -- or null
  int32_t* chunk;            // (n_views, n_chunks) out: exclusive offsets per 1024-point chunk (k_mask_chunk_scan's table)
  int n_tiles, n_chunks, n_views;   // n_tiles: row stride of tile_cnt (= 4 n_chunks)
  int n_real;                       // tiles the cloud really has: ceil(n / 256)
  int64_t* first; int64_t* num; int32_t* view_total;
};
__device__ void chunk_scan_job(const ChunkScanJob& j);

// imported halo records (N ranks): the LAST `blocks` workgroups of the count / scatter launch take them (launches of their
// own were 8 + 6 us per grid at the size of a rank's share of eight); blocks == 0: none
struct ImportJob { const float4* rec0; const float4* rec1; const int32_t* count; int64_t max; int blocks; };

__global__ __launch_bounds__(256) void k_brick_count(const float* __restrict__ pts, int64_t n,
                                                     BrickHdr* __restrict__ hp, int32_t* __restrict__ cnt,
                                                     int32_t* __restrict__ slot, int pending, BrickParams q,
                                                     int32_t* __restrict__ counters, ChunkScanJob job, ImportJob imp) {
  __shared__ int t_key[kCntTab], t_cnt[kCntTab];
  __shared__ BrickHdr s_h;
  if (imp.blocks && (int)blockIdx.x >= (int)gridDim.x - imp.blocks) {      // (only with a header that is already written)
    const int bid = (int)blockIdx.x - ((int)gridDim.x - imp.blocks);
    const BrickHdr h = *hp;
    int64_t m = *imp.count;
    if (m > imp.max) m = imp.max;
    if (bid == 0 && threadIdx.x == 0) hp->n = h.n_own + (int)m;
    for (int64_t base = (int64_t)bid * 1024; base < m; base += (int64_t)imp.blocks * 1024)
      brick_count_round(h, base, m, cnt, slot + h.n_own, t_key, t_cnt,
                        [&](int64_t j, int, float& x, float& y, float& z) { const float4 p = imp.rec0[j]; x = p.x; y = p.y; z = p.z; });
    return;
  }
  const bool scan_wg = job.chunk && blockIdx.x == 0;
  if (scan_wg && gridDim.x > 1) { chunk_scan_job(job); return; }        // (needs no header; another workgroup stores it)
  if (pending) {
    __shared__ unsigned s_red[8];
    float mn[3], mx[3];
    bk_box_read(counters, s_red, mn, mx);
    if (threadIdx.x == 0) {
      s_h = bricks_header(mn, mx, q);
      if (blockIdx.x == gridDim.x - 1) bricks_store_header(s_h, hp, counters);
    }
    __syncthreads();
  }
  if (scan_wg) { chunk_scan_job(job); return; }
  const BrickHdr h = pending ? s_h : *hp;
  const int n_wg = (int)gridDim.x - imp.blocks - (job.chunk ? 1 : 0);
  // (the scan job, if any, is workgroup 0: it has the longest chain of dependent steps of the launch and starts first)
  for (int64_t base = (int64_t)(blockIdx.x - (job.chunk ? 1 : 0)) * 1024; base < n; base += (int64_t)n_wg * 1024)
    brick_count_round(h, base, n, cnt, slot, t_key, t_cnt,
                      [&](int64_t i, int, float& x, float& y, float& z) { x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2]; });
}

// imported halo records (count on the device); same aggregation
__global__ __launch_bounds__(256) void k_brick_count_recs(const float4* __restrict__ imp0, const int32_t* __restrict__ imp_count,
                                                          int64_t imp_max, BrickHdr* __restrict__ hp,
                                                          int32_t* __restrict__ cnt, int32_t* __restrict__ slot) {
  __shared__ int t_key[kCntTab], t_cnt[kCntTab];
  const BrickHdr h = *hp;
  int64_t m = *imp_count;
  if (m > imp_max) m = imp_max;
  if (blockIdx.x == 0 && threadIdx.x == 0) hp->n = h.n_own + (int)m;
  for (int64_t base = (int64_t)blockIdx.x * 1024; base < m; base += (int64_t)gridDim.x * 1024)
    brick_count_round(h, base, m, cnt, slot + h.n_own, t_key, t_cnt,
                      [&](int64_t j, int, float& x, float& y, float& z) { const float4 p = imp0[j]; x = p.x; y = p.y; z = p.z; });
}

__global__ __launch_bounds__(256) void k_brick_scatter(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                       const int32_t* __restrict__ payload, int64_t n,
                                                       const BrickHdr* __restrict__ hp, const int32_t* __restrict__ off,
                                                       const int32_t* __restrict__ slot, float4* __restrict__ rec0,
                                                       float4* __restrict__ rec1, ImportJob imp) {
  const BrickHdr h = *hp;
  if (imp.blocks && (int)blockIdx.x >= (int)gridDim.x - imp.blocks) {
    const int bid = (int)blockIdx.x - ((int)gridDim.x - imp.blocks);
    const int64_t m = h.n - h.n_own;
    for (int64_t j = (int64_t)bid * blockDim.x + threadIdx.x; j < m; j += (int64_t)imp.blocks * blockDim.x) {
      const float4 p = imp.rec0[j];
      const int64_t dst = (int64_t)off[counter_of(h, p.x, p.y, p.z)] + slot[h.n_own + j];
      rec0[dst] = p;
      float4 u = imp.rec1[j];                              // an exported record carries the raw normal
      bk_unit_normal(u.x, u.y, u.z);
      rec1[dst] = u;
    }
    return;
  }
  const int n_wg = (int)gridDim.x - imp.blocks;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)n_wg * blockDim.x) {
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    const int64_t dst = (int64_t)off[counter_of(h, x, y, z)] + slot[i];            // slot: rank inside the counter (k_brick_count)
    rec0[dst] = make_float4(x, y, z, __int_as_float(h.id_base + (int)i));
    float4 u = make_float4(0.f, 0.f, 0.f, __int_as_float(payload ? payload[i] : 0));
    if (nrm) { u.x = nrm[i * 3]; u.y = nrm[i * 3 + 1]; u.z = nrm[i * 3 + 2]; bk_unit_normal(u.x, u.y, u.z); }
    rec1[dst] = u;
  }
}

__global__ __launch_bounds__(256) void k_brick_scatter_recs(const float4* __restrict__ imp0, const float4* __restrict__ imp1,
                                                            const BrickHdr* __restrict__ hp, const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ slot, float4* __restrict__ rec0,
                                                            float4* __restrict__ rec1) {
  const BrickHdr h = *hp;
  const int64_t m = h.n - h.n_own;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = imp0[j];
    const int64_t dst = (int64_t)off[counter_of(h, p.x, p.y, p.z)] + slot[h.n_own + j];
    rec0[dst] = p;
    float4 u = imp1[j];                                  // an exported record carries the raw normal
    bk_unit_normal(u.x, u.y, u.z);
    rec1[dst] = u;
  }
}

// ---- offsets of the bricks: exclusive scan of the counters in two launches ---------------------------
// (the general 3-phase scan of frnn.hip, specialised: a table of <= ~2000 chunks needs no middle pass -- every
// block of the second pass adds up the totals of the chunks before it -- and the second pass also does what two
// more launches did: it leaves the counters ZEROED for the next build and appends the occupied bricks to the work
// list, one returning atomic per 2048 bricks; the order of the list only affects scheduling.)
// The unit of the scan is the BRICK: a chunk is BS_CHUNK bricks (a thread takes BS_ITEMS of them, BK_CPB counters each, as
// 16-byte loads), so that the number of chunks -- and of workgroups that wait for one another in the one-launch form -- stays
// <= 2001 whatever BK_CPB is.
constexpr int BS_ITEMS = 4, BS_CHUNK = 256 * BS_ITEMS;
static_assert(BK_CPB == 8, "a brick's counters are two 16-byte words");

// a thread's BS_ITEMS bricks of chunk `chunk`: their counters (zeroed behind the read when ZERO) and the brick totals
template <bool ZERO>
__device__ __forceinline__ int brick_counters_load(int32_t* __restrict__ cnt, int chunk, int nb, int (&c)[BS_ITEMS][BK_CPB],
                                                   int (&tot)[BS_ITEMS]) {
  int v = 0;
#pragma unroll
  for (int k = 0; k < BS_ITEMS; ++k) {
    const int brick = chunk * BS_CHUNK + threadIdx.x * BS_ITEMS + k;
    tot[k] = 0;
#pragma unroll
    for (int q = 0; q < BK_CPB; ++q) c[k][q] = 0;
    if (brick < nb) {
      int4* p = reinterpret_cast<int4*>(cnt + (int64_t)BK_CPB * brick);
      const int4 a = p[0], b = p[1];
      c[k][0] = a.x; c[k][1] = a.y; c[k][2] = a.z; c[k][3] = a.w; c[k][4] = b.x; c[k][5] = b.y; c[k][6] = b.z; c[k][7] = b.w;
      if (ZERO) { p[0] = make_int4(0, 0, 0, 0); p[1] = make_int4(0, 0, 0, 0); }
#pragma unroll
      for (int q = 0; q < BK_CPB; ++q) tot[k] += c[k][q];
    }
    v += tot[k];
  }
  return v;
}
// offsets of those bricks' counters from the exclusive prefix `ex` of the thread, occupied bricks appended at list[at..]
__device__ __forceinline__ void brick_offsets_store(int32_t* __restrict__ off, int32_t* __restrict__ list, int chunk, int nb,
                                                    const int (&c)[BS_ITEMS][BK_CPB], const int (&tot)[BS_ITEMS], int ex, int at,
                                                    const bool (&listed)[BS_ITEMS]) {
#pragma unroll
  for (int k = 0; k < BS_ITEMS; ++k) {
    const int brick = chunk * BS_CHUNK + threadIdx.x * BS_ITEMS + k;
    if (brick < nb) {
      int o[BK_CPB];
#pragma unroll
      for (int q = 0; q < BK_CPB; ++q) { o[q] = ex; ex += c[k][q]; }
      int4* p = reinterpret_cast<int4*>(off + (int64_t)BK_CPB * brick);
      p[0] = make_int4(o[0], o[1], o[2], o[3]);
      p[1] = make_int4(o[4], o[5], o[6], o[7]);
      if (listed[k]) list[at++] = brick;
    } else if (brick == nb) {
      off[(int64_t)BK_CPB * nb] = ex;                    // the sentinel behind the last brick
    }
  }
}

// bricks of the work list: occupied, and in a brick column (x-major brick ids) that can hold points of this rank
__device__ __forceinline__ void brick_listed(const BrickHdr& h, int chunk, const int (&tot)[BS_ITEMS], bool (&listed)[BS_ITEMS]) {
  const int per_col = h.nb[1] * h.nb[2];
#pragma unroll
  for (int k = 0; k < BS_ITEMS; ++k) {
    const int brick = chunk * BS_CHUNK + threadIdx.x * BS_ITEMS + k;
    const int bx = brick / per_col;
    listed[k] = tot[k] > 0 && bx >= h.own_bx_lo && bx <= h.own_bx_hi;
  }
}

__global__ __launch_bounds__(256) void k_brick_sums(const BrickHdr* __restrict__ hp, int32_t* __restrict__ cnt,
                                                    int32_t* __restrict__ sums) {
  __shared__ int lds[4];
  const int nb = hp->n_bricks;
  if ((int)blockIdx.x * BS_CHUNK > nb) return;
  int c[BS_ITEMS][BK_CPB], t[BS_ITEMS];
  const int v = brick_counters_load<false>(cnt, blockIdx.x, nb, c, t);
  int tot;
  iso_block_excl_scan<4>(v, tot, lds);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_brick_offsets(const BrickHdr* __restrict__ hp, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ off, const int32_t* __restrict__ sums,
                                                       int32_t* __restrict__ list, int32_t* __restrict__ counters) {
  __shared__ int lds[4], s_base;
  const int nb = hp->n_bricks;
  if ((int)blockIdx.x * BS_CHUNK > nb) return;           // (chunk nb / BS_CHUNK also holds the sentinel)
  if (blockIdx.x == 0) bk_box_clear(counters);
  int before = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += 256) before += sums[i];
  int base;
  iso_block_excl_scan<4>(before, base, lds);                       // base = total of the chunks before this one
  int c[BS_ITEMS][BK_CPB], t[BS_ITEMS];
  const int v = brick_counters_load<true>(cnt, blockIdx.x, nb, c, t);
  int occ = 0;
  bool listed[BS_ITEMS];
  brick_listed(*hp, blockIdx.x, t, listed);
#pragma unroll
  for (int k = 0; k < BS_ITEMS; ++k) occ += listed[k] ? 1 : 0;
  int tot, occ_tot;
  const int ex = base + iso_block_excl_scan<4>(v, tot, lds);
  int at = iso_block_excl_scan<4>(occ, occ_tot, lds);
  if (threadIdx.x == 0) s_base = occ_tot ? atomicAdd(&counters[0], occ_tot) : 0;
  __syncthreads();
  brick_offsets_store(off, list, blockIdx.x, nb, c, t, ex, at + s_base, listed);
}

// The two passes above as ONE launch (2048 workgroups of this size are resident at once -- 8 per CU --, so a workgroup may
// wait for the ones before it; BK_NB_MAX bricks per axis are <= 4001 chunks of which the first <= 2048 do the waiting: the
// host takes the two-launch form beyond): a workgroup publishes its chunk total (bit 31 = "there") with an agent-scope
// store, adds up the totals of the chunks before it as they appear (polled by 256 lanes), and goes on as k_brick_offsets
// does.  The workgroup that finishes last clears the totals: `sums` is zero on entry and zero again on exit
// (iso_bricks_workspace_init clears it once).
constexpr int kScan1Max = 2048;
static_assert(kScan1Max == kScan1MaxWords, "bricks_carve sizes the zeroed words");
__global__ __launch_bounds__(256) void k_brick_offsets1(const BrickHdr* __restrict__ hp, int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ off, unsigned* __restrict__ sums,
                                                        int32_t* __restrict__ list, int32_t* __restrict__ counters) {
  __shared__ int lds[4], s_base, s_last;
  const int nb = hp->n_bricks;
  if ((int)blockIdx.x * BS_CHUNK > nb) return;
  if (blockIdx.x == 0) bk_box_clear(counters);      // every reader of the pending box (the count pass) is done
  const int n_active = nb / BS_CHUNK + 1;
  int c[BS_ITEMS][BK_CPB], t[BS_ITEMS];
  const int v = brick_counters_load<true>(cnt, blockIdx.x, nb, c, t);
  int occ = 0;
  bool listed[BS_ITEMS];
  brick_listed(*hp, blockIdx.x, t, listed);
#pragma unroll
  for (int k = 0; k < BS_ITEMS; ++k) occ += listed[k] ? 1 : 0;
  int tot, occ_tot;
  int ex = iso_block_excl_scan<4>(v, tot, lds);
  if (threadIdx.x == 0) __hip_atomic_store(&sums[blockIdx.x], 0x80000000u | (unsigned)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int before = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += 256) {
    unsigned q;
    while (!((q = __hip_atomic_load(&sums[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0x80000000u)) __builtin_amdgcn_s_sleep(1);
    before += (int)(q & 0x7fffffffu);
  }
  int base;
  iso_block_excl_scan<4>(before, base, lds);                       // base = total of the chunks before this one
  ex += base;
  int at = iso_block_excl_scan<4>(occ, occ_tot, lds);
  if (threadIdx.x == 0) s_base = occ_tot ? atomicAdd(&counters[0], occ_tot) : 0;
  __syncthreads();
  brick_offsets_store(off, list, blockIdx.x, nb, c, t, ex, at + s_base, listed);
  // everyone has read the totals it needs once it is here; the last one clears them
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* arrive = reinterpret_cast<unsigned*>(counters) + kArriveAt;
    const unsigned prev = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == (unsigned)n_active - 1u;
    if (s_last) __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_last)
    for (int i = threadIdx.x; i < n_active; i += 256) __hip_atomic_store(&sums[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The chunk scan of the splat front end (k_mask_chunk_scan in splat.hip: exclusive scan of every view's per-chunk counts,
// first_idx / num_points as the packed layout of _C.splat_points takes them, view totals) by ONE workgroup of 256 that
// rides in the count launch of the grid the front end needs anyway.  The counts come per 256-point tile (four tiles per
// chunk) from the launch that took the mask (follow.h).
__device__ void chunk_scan_job(const ChunkScanJob& j) {
  __shared__ int s_tot[8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // a WAVE per view (no workgroup barrier inside the scan): a lane takes four consecutive chunks per step -- sixteen tile
  // counts, four 16-byte loads, all requested before the first is used -- and the wave scans 256 chunks per step
  for (int v = w; v < j.n_views; v += 4) {
    const int32_t* tc = j.tile_cnt + (int64_t)v * j.n_tiles;
    int32_t* row = j.chunk + (int64_t)v * j.n_chunks;
    int carry = 0;
    for (int c0 = 0; c0 < j.n_chunks; c0 += 256) {
      int val[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = c0 + 4 * lane + q;
        val[q] = 0;
        if (i < j.n_chunks) {
          if (4 * i + 3 < j.n_real) { const int4 c = *reinterpret_cast<const int4*>(tc + 4 * i); val[q] = (c.x + c.y) + (c.z + c.w); }
          else for (int k = 0; 4 * i + k < j.n_real; ++k) val[q] += tc[4 * i + k];
        }
      }
      const int mine = (val[0] + val[1]) + (val[2] + val[3]);
      int inc = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
      int ex = carry + inc - mine;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = c0 + 4 * lane + q;
        if (i < j.n_chunks) row[i] = ex;
        ex += val[q];
      }
      carry += __shfl(inc, 63);
    }
    if (lane == 0) s_tot[v] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int v = 0; v < j.n_views; ++v) { j.first[v] = run; j.num[v] = s_tot[v]; j.view_total[v] = s_tot[v]; run += s_tot[v]; }
    for (int v = j.n_views; v < 8; ++v) j.view_total[v] = 0;
  }
}

}  // namespace

// ================================================================================================
extern "C" int64_t iso_bricks_workspace_bytes(int64_t n_max) {
  return bricks_carve(nullptr, n_max).bytes;
}

extern "C" int iso_bricks_workspace_init(void* workspace, int64_t n_max, void* stream) {
  ISO_REQUIRE(workspace && n_max >= 0, ISO_ERR_INVALID, "iso_bricks_workspace_init: bad arguments");
  ISO_REQUIRE(((uintptr_t)workspace & 255) == 0, ISO_ERR_INVALID, "iso_bricks_workspace_init: workspace must be 256-B aligned");
  const BrickWs w = bricks_carve(workspace, n_max);
  hipLaunchKernelGGL(k_bricks_init, dim3(iso_stream_grid(w.G, 256)), dim3(256), 0, (hipStream_t)stream, w.counters, w.cnt, w.G, w.scan1);
  ISO_CHECK_LAUNCH("iso_bricks_workspace_init");
  return ISO_OK;
}

// Diagnostic (synchronises the stream): did iso_bricks_workspace_init ever run on this workspace?  A build on a workspace
// that was never initialised counts into whatever the memory held and produces a wrong grid without any other sign.
extern "C" int iso_bricks_workspace_check(const void* workspace, int64_t n_max, void* stream) {
  ISO_REQUIRE(workspace && n_max >= 0, ISO_ERR_INVALID, "iso_bricks_workspace_check: bad arguments");
  ISO_REQUIRE(((uintptr_t)workspace & 255) == 0, ISO_ERR_INVALID, "iso_bricks_workspace_check: workspace must be 256-B aligned");
  const BrickWs w = bricks_carve(const_cast<void*>(workspace), n_max);
  // the counter block up to the pending box + the chunk totals of the one-launch scan (both at fixed offsets)
  int32_t host[kBoxAt + kScan1MaxWords];                  // per call (a static one raced between host threads: ADVICE r5)
  ISO_REQUIRE(hipMemcpyAsync(host, w.counters, 4 * kBoxAt, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess &&
                  hipMemcpyAsync(host + kBoxAt, w.scan1, 4 * kScan1MaxWords, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess &&
                  hipStreamSynchronize((hipStream_t)stream) == hipSuccess,
              ISO_ERR_LAUNCH, "iso_bricks_workspace_check: could not read the workspace");
  ISO_REQUIRE(host[kMagicAt] == kBrickMagic, ISO_ERR_INVALID,
              "iso_bricks_workspace_check: the workspace was never initialised (iso_bricks_workspace_init)");
  // what the builds rely on finding zero (an aborted launch, or a build on dirty memory, leaves them set and every later
  // build on the workspace then computes wrong offsets): the arrival words and the scan's chunk totals
  for (int i = kArriveAt; i < kArriveAt + 17; ++i)
    ISO_REQUIRE(host[i] == 0, ISO_ERR_INVALID, "iso_bricks_workspace_check: arrival word %d is not zero (an aborted build?): "
                "re-initialise the workspace", i - kArriveAt);
  for (int i = 0; i < kScan1MaxWords; ++i)
    ISO_REQUIRE(host[kBoxAt + i] == 0, ISO_ERR_INVALID, "iso_bricks_workspace_check: chunk total %d of the brick scan is not zero "
                "(an aborted build?): re-initialise the workspace", i);
  return ISO_OK;
}

// count -> offsets (+ work list, counters left zeroed) -> scatter, on a header that is already written
static int bricks_fill(const BrickWs& w, const float* points, const float* normals, const int32_t* payload, int64_t n_own,
                       const float* import_rec0, const float* import_rec1, const int32_t* import_count,
                       int64_t import_max, hipStream_t s, bool pending = false, BrickParams q = BrickParams{0, 0, 0, 0.f, 0, 0.f, 0},
                       ChunkScanJob job = ChunkScanJob{nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr}) {
  // imported records ride in the launches of the own points when the header is there already (the N-rank path: it is
  // written before the halo exchange)
  const bool ride = import_max > 0 && n_own > 0 && !pending && !job.chunk;
  const ImportJob none{nullptr, nullptr, nullptr, 0, 0};
  const ImportJob imp_c{(const float4*)import_rec0, (const float4*)import_rec1, import_count, import_max,
                        ride ? iso_stream_grid(import_max, 1024) : 0};
  const ImportJob imp_s{(const float4*)import_rec0, (const float4*)import_rec1, import_count, import_max,
                        ride ? iso_stream_grid(import_max, 256) : 0};
  if (n_own > 0 || pending || job.chunk)        // (a pending header is written by this pass, whatever the cloud holds)
    hipLaunchKernelGGL(k_brick_count, dim3(iso_stream_grid(n_own, 1024) + (job.chunk ? 1 : 0) + imp_c.blocks), dim3(256), 0, s,
                       points, n_own, w.hdr, w.cnt, w.slot, pending ? 1 : 0, q, w.counters, job, ride ? imp_c : none);
  if (import_max > 0 && !ride)
    hipLaunchKernelGGL(k_brick_count_recs, dim3(iso_stream_grid(import_max, 1024)), dim3(256), 0, s,
                       (const float4*)import_rec0, import_count, import_max, w.hdr, w.cnt, w.slot);
  const int chunks = (int)(((w.G - 1) / BK_CPB + 1 + BS_CHUNK - 1) / BS_CHUNK);      // chunks of BS_CHUNK bricks (+ the sentinel)
  ISO_REQUIRE(w.scan_ws_bytes >= (int64_t)(chunks + kScan1Max) * 4, ISO_ERR_WORKSPACE, "iso_bricks_build: scan workspace too small");
  if (chunks <= kScan1Max) {            // one launch (the totals are zero on entry and left zero)
    hipLaunchKernelGGL(k_brick_offsets1, dim3(chunks), dim3(256), 0, s, w.hdr, w.cnt, w.off, w.scan1, w.list,
                       w.counters);
  } else {
    int32_t* sums2 = (int32_t*)w.scan_ws + kScan1Max;       // (behind the words the one-launch form keeps zeroed)
    hipLaunchKernelGGL(k_brick_sums, dim3(chunks), dim3(256), 0, s, w.hdr, w.cnt, sums2);
    hipLaunchKernelGGL(k_brick_offsets, dim3(chunks), dim3(256), 0, s, w.hdr, w.cnt, w.off, (const int32_t*)sums2, w.list,
                       w.counters);
  }
  if (n_own > 0)
    hipLaunchKernelGGL(k_brick_scatter, dim3(iso_stream_grid(n_own, 256) + imp_s.blocks), dim3(256), 0, s, points, normals, payload,
                       n_own, w.hdr, w.off, w.slot, w.rec0, w.rec1, ride ? imp_s : none);
  if (import_max > 0 && !ride)
    hipLaunchKernelGGL(k_brick_scatter_recs, dim3(iso_stream_grid(import_max, 256)), dim3(256), 0, s,
                       (const float4*)import_rec0, (const float4*)import_rec1, w.hdr, w.off, w.slot, w.rec0, w.rec1);
  return ISO_OK;
}

extern "C" int iso_bricks_build(const float* points, const float* normals, const int32_t* payload,
                                int64_t n_own, int64_t id_base, const float* import_rec0,
                                const float* import_rec1, const int32_t* import_count, int64_t import_max,
                                const float* bbox, int64_t n_total, float radius, int knn_k,
                                float cell_scale, void* workspace, int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(n_own >= 0 && import_max >= 0 && n_total >= 0, ISO_ERR_INVALID, "iso_bricks_build: bad sizes");
  ISO_REQUIRE(workspace && (points || n_own == 0), ISO_ERR_INVALID, "iso_bricks_build: null pointer");
  ISO_REQUIRE(import_max == 0 || (import_rec0 && import_rec1 && import_count), ISO_ERR_INVALID,
              "iso_bricks_build: import buffers missing");
  ISO_REQUIRE(cell_scale > 0.f && (radius > 0.f || knn_k > 0), ISO_ERR_INVALID,
              "iso_bricks_build: cell_scale and radius / knn_k must be positive");
  ISO_REQUIRE(((uintptr_t)workspace & 255) == 0, ISO_ERR_INVALID, "iso_bricks_build: workspace must be 256-B aligned");
  const int64_t n_max = n_own + import_max;
  ISO_REQUIRE(id_base + n_max < (1ll << 28), ISO_ERR_UNSUPPORTED, "iso_bricks_build: ids must stay below 2^28");
  const BrickWs w = bricks_carve(workspace, n_max);
  ISO_REQUIRE(workspace_bytes >= w.bytes, ISO_ERR_WORKSPACE, "iso_bricks_build: workspace too small (%lld < %lld)",
              (long long)workspace_bytes, (long long)w.bytes);
  hipStream_t s = (hipStream_t)stream;
  if (bbox)        // NULL: the header was written by iso_bricks_params (N ranks: between it and here the halo exchange)
    hipLaunchKernelGGL(k_bricks_params, dim3(1), dim3(64), 0, s, bbox, 1,
                       BrickParams{n_total, n_own, id_base, radius, knn_k, cell_scale, w.nb_cap}, w.hdr, w.counters);
  int rc = bricks_fill(w, points, normals, payload, n_own, import_rec0, import_rec1, import_count, import_max, s);
  if (rc != ISO_OK) return rc;
  ISO_CHECK_LAUNCH("iso_bricks_build");
  return ISO_OK;
}

static int build_whole_checks(const char* who, const float* points, int64_t n, float radius, int knn_k, float cell_scale,
                              void* workspace, int64_t workspace_bytes, BrickWs& w) {
  ISO_REQUIRE(n >= 0 && workspace && (points || n == 0), ISO_ERR_INVALID, "%s: bad arguments", who);
  ISO_REQUIRE(cell_scale > 0.f && (radius > 0.f || knn_k > 0), ISO_ERR_INVALID,
              "%s: cell_scale and radius / knn_k must be positive", who);
  ISO_REQUIRE(((uintptr_t)workspace & 255) == 0, ISO_ERR_INVALID, "%s: workspace must be 256-B aligned", who);
  ISO_REQUIRE(n < (1ll << 28), ISO_ERR_UNSUPPORTED, "%s: ids must stay below 2^28", who);
  w = bricks_carve(workspace, n);
  ISO_REQUIRE(workspace_bytes >= w.bytes, ISO_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld)", who,
              (long long)workspace_bytes, (long long)w.bytes);
  return ISO_OK;
}

extern "C" int iso_bricks_build_whole(const float* points, const float* normals, const int32_t* payload, int64_t n,
                                      float radius, int knn_k, float cell_scale, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  BrickWs w;
  int rc = build_whole_checks("iso_bricks_build_whole", points, n, radius, knn_k, cell_scale, workspace, workspace_bytes, w);
  if (rc != ISO_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    int gx = iso_div_up(n * 3, 256 * 4);       // four loads per thread and round; a stride of a multiple of 3 floats
    if (gx > 1023) gx = 1023;
    if (gx >= 3) gx -= gx % 3; else gx = 3;
    hipLaunchKernelGGL(k_brick_bbox, dim3(gx), dim3(256), 0, s, points, n, w.counters);
  }
  rc = bricks_fill(w, points, normals, payload, n, nullptr, nullptr, nullptr, 0, s, true,
                   BrickParams{n, n, 0, radius, knn_k, cell_scale, w.nb_cap});
  if (rc != ISO_OK) return rc;
  ISO_CHECK_LAUNCH("iso_bricks_build_whole");
  return ISO_OK;
}

extern "C" int iso_bricks_build_pending(const float* points, const float* normals, const int32_t* payload, int64_t n,
                                        float radius, int knn_k, float cell_scale, void* workspace,
                                        int64_t workspace_bytes, const iso_follow* f, void* stream) {
  BrickWs w;
  int rc = build_whole_checks("iso_bricks_build_pending", points, n, radius, knn_k, cell_scale, workspace, workspace_bytes, w);
  if (rc != ISO_OK) return rc;
  ChunkScanJob job{nullptr, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr};
  if (f && f->views) {
    ISO_REQUIRE(f->n_views >= 1 && f->n_views <= 8 && f->front_ws && f->first_idx_out && f->num_pts_out && f->view_total_out,
                ISO_ERR_INVALID, "iso_bricks_build_pending: follow: mask part incomplete");
    ISO_REQUIRE(f->front_ws_bytes >= iso_splat_front_workspace_bytes(n), ISO_ERR_WORKSPACE,
                "iso_bricks_build_pending: follow.front_ws too small");
    job.n_chunks = (int)((n + 1023) / 1024);
    job.n_tiles = 4 * job.n_chunks;                     // row stride of the tile table (follow.h)
    job.n_real = (int)((n + 255) / 256);
    job.n_views = f->n_views;
    job.tile_cnt = front_tile_table(f->front_ws, n);
    job.chunk = (int32_t*)f->front_ws;
    job.first = f->first_idx_out; job.num = f->num_pts_out; job.view_total = f->view_total_out;
  }
  rc = bricks_fill(w, points, normals, payload, n, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, true,
                   BrickParams{n, n, 0, radius, knn_k, cell_scale, w.nb_cap}, job);
  if (rc != ISO_OK) return rc;
  ISO_CHECK_LAUNCH("iso_bricks_build_pending");
  return ISO_OK;
}

extern "C" int iso_bricks_box_take(void* workspace, int64_t n_max, float* box_out, void* stream) {
  ISO_REQUIRE(workspace && box_out && n_max >= 0, ISO_ERR_INVALID, "iso_bricks_box_take: bad arguments");
  const BrickWs w = bricks_carve(workspace, n_max);
  hipLaunchKernelGGL(k_brick_box_take, dim3(1), dim3(256), 0, (hipStream_t)stream, w.counters, box_out);
  ISO_CHECK_LAUNCH("iso_bricks_box_take");
  return ISO_OK;
}

extern "C" int iso_bricks_params(const float* boxes, int n_boxes, int64_t n_total, int64_t n_own, int64_t id_base,
                                 float radius, int knn_k, float cell_scale, void* workspace, int64_t n_max, void* stream) {
  ISO_REQUIRE(boxes && n_boxes >= 1 && workspace && n_max >= n_own && n_own >= 0 && n_total >= 0, ISO_ERR_INVALID,
              "iso_bricks_params: bad arguments");
  ISO_REQUIRE(cell_scale > 0.f && (radius > 0.f || knn_k > 0), ISO_ERR_INVALID,
              "iso_bricks_params: cell_scale and radius / knn_k must be positive");
  const BrickWs w = bricks_carve(workspace, n_max);
  hipLaunchKernelGGL(k_bricks_params, dim3(1), dim3(64), 0, (hipStream_t)stream, boxes, n_boxes,
                     BrickParams{n_total, n_own, id_base, radius, knn_k, cell_scale, w.nb_cap}, w.hdr, w.counters);
  ISO_CHECK_LAUNCH("iso_bricks_params");
  return ISO_OK;
}
