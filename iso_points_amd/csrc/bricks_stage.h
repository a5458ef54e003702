// What the two fused kernels of the brick grid share (k_brick_resample in bricks_resample.hip, k_brick_h in bricks_h.hip):
// level 2 of bricks.h -- a workgroup stages one brick + a fine cell of halo into LDS, counting-sorted by local cell, and
// its queries walk windows of that block --, the hand-over of a brick that does not fit to the tail kernels
// (bricks_walk.h), which brick of the work list a workgroup takes, and the size of the grids.  Private to csrc/.
#pragma once
#include "bricks.h"

#pragma clang fp contract(off)

namespace {

// ---- staging of one brick + halo into LDS -------------------------------------------------------
// WITH_NRM: rec1 (normals) staged next to rec0 (resample); otherwise one record per candidate whose
// w is rec1's payload (the view mask) with bit 31 = "imported, not a query" (bandwidth kernel).
// SUB: the LDS sort runs on SUB x SUB x SUB sub-cells per fine cell (the global grid and everything outside the
// workgroup know fine cells only).  SUB = 2 (resample): a query walks a 4 x 4 x 4 window of HALF cells picked by the
// half of its own half cell it lies in -- every point within 0.75 fine cells of the query is inside (1.5 half cells to
// each face), 1.6 r wide at the 0.8 r cell against the 2.4 r of a 3 x 3 x 3 walk of whole cells: 44 % of the candidates.
// Runs of the brick-sorted arrays a workgroup stages: per (x slot, y slot, neighbour in z) the sub-bricks that touch the
// brick -- x slot 0..3 = (brick x - 1, sub x 1), (x, 0), (x, 1), (x + 1, 0); same in y; in z the whole sub-brick column of
// the brick itself, the upper sub-bricks of the one below, the lower ones of the one above.
constexpr int kStageRuns = 48;
template <bool WITH_NRM, int SUB = 1, int CAP = BK_CAP>
struct BrickStage {
  static constexpr int NL = 6 * SUB;                // local (sub-)cells per axis: the brick + one fine cell of halo
  static constexpr int NCELL = NL * NL * NL;
  static constexpr int NQRUN = 16 * SUB * SUB;      // z-runs of the brick's own (sub-)cells
  float4 rec0[CAP];
  int src[WITH_NRM ? CAP : 1];     // WITH_NRM: position of the staged record in the brick-sorted arrays (its rec1 is read
                                      // from there by the few that need it: staging it cost 16 KB of LDS = three workgroups per CU)
  int gid[WITH_NRM ? 1 : CAP];
  int cstart[NCELL + 4];   // [NCELL + 1] used: local (sub-)cell -> first staged slot
  int ccur[NCELL];
  int run_i0[kStageRuns];
  int run_pre[kStageRuns + 1];
  int qbeg[NQRUN];
  int qpre[NQRUN + 1];
};

struct BrickGeo { int bx, by, bz, ox, oy, oz; };

// All threads of the workgroup.  Returns the number of staged records, or -1 when they do not fit.
// The records of the 27 bricks are nine contiguous runs of the brick-sorted arrays; a thread takes
// every BK_THREADS-th record of their concatenation and requests all of its records before it uses
// the first (BK_RAW in flight: the staging is a chain of global-memory latencies otherwise).
constexpr int BK_RAW = 8;

// VS (bandwidth kernel only): bit stride of the view mask in the staged record -- 1: as stored; 8: view v at bit
// 8 v (up to four views), so that masked records add up to four 8-bit per-view counters in one register.
template <bool WITH_NRM, int VS = 1, int SUB = 1, int CAP = BK_CAP>
__device__ int stage_brick(BrickStage<WITH_NRM, SUB, CAP>& S, const BrickHdr& h, const int32_t* __restrict__ off,
                           const float4* __restrict__ rec0, const float4* __restrict__ rec1, int b, BrickGeo& g) {
  typedef BrickStage<WITH_NRM, SUB, CAP> St;
  constexpr int NL = St::NL, NCELL = St::NCELL;
  const int tid = threadIdx.x;
  const int nbx = h.nb[0], nby = h.nb[1], nbz = h.nb[2];
  g.bz = b % nbz; g.by = (b / nbz) % nby; g.bx = b / (nbz * nby);
  g.ox = 4 * g.bx - 1; g.oy = 4 * g.by - 1; g.oz = 4 * g.bz - 1;
  __syncthreads();                                   // the previous brick's readers are done
  for (int c = tid; c < NCELL; c += BK_THREADS) S.ccur[c] = 0;
  if (tid < kStageRuns) {
    // (rt: the thread index behind an opaque move -- the run's offsets below depend on the thread only, so the compiler
    // hoists them out of the caller's brick loop and then SPILLS them across it: five scratch registers in
    // k_brick_resample, eight in k_brick_h, reloaded once per brick; recomputing 48 lanes' worth per brick is free)
    int rt = tid;
    asm volatile("" : "+v"(rt));
    const int xs = rt / 12, ys = (rt / 3) % 4, dz = rt % 3 - 1;
    const int x = g.bx + (xs + 1) / 2 - 1, sx = xs == 0 ? 1 : (xs == 3 ? 0 : xs - 1);      // xs 0..3 -> (dx, sub x) = (-1,1) (0,0) (0,1) (+1,0)
    const int y = g.by + (ys + 1) / 2 - 1, sy = ys == 0 ? 1 : (ys == 3 ? 0 : ys - 1);
    const int z = g.bz + dz;
    int i0 = 0, len = 0;
    if (x >= 0 && x < nbx && y >= 0 && y < nby && z >= 0 && z < nbz) {
      const int c = BK_CPB * ((x * nby + y) * nbz + z) + (sx * 2 + sy) * 2;
      const int lo = dz < 0 ? 1 : 0, hi = dz > 0 ? 0 : 1;                // sub z: both of the own brick, the near one of a neighbour
      i0 = off[c + lo];
      len = off[c + hi + 1] - i0;
    }
    S.run_i0[tid] = i0;
    S.run_pre[tid + 1] = len;
  }
  __syncthreads();
  if (tid < 64) {                                    // exclusive prefix of the run lengths (one wave)
    const int len = tid < kStageRuns ? S.run_pre[tid + 1] : 0;
    const int inc = iso_wave_incl_scan(len);
    if (tid < kStageRuns) S.run_pre[tid + 1] = inc;
    if (tid == 0) S.run_pre[0] = 0;
  }
  __syncthreads();
  const int total_raw = S.run_pre[kStageRuns];
  auto index_of = [&](int j) {                       // the run r with run_pre[r] <= j < run_pre[r + 1]
    int lo = 0, hi = kStageRuns;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (S.run_pre[mid] <= j) lo = mid; else hi = mid;
    }
    return S.run_i0[lo] + (j - S.run_pre[lo]);
  };
  auto cell_of = [&](const float4& p) {
    const int lx = bk_sub<SUB>(p.x, h.mn[0], h.inv_f, h.nf[0]) - SUB * g.ox;
    const int ly = bk_sub<SUB>(p.y, h.mn[1], h.inv_f, h.nf[1]) - SUB * g.oy;
    const int lz = bk_sub<SUB>(p.z, h.mn[2], h.inv_f, h.nf[2]) - SUB * g.oz;
    return ((unsigned)lx < (unsigned)NL && (unsigned)ly < (unsigned)NL && (unsigned)lz < (unsigned)NL) ? (lx * NL + ly) * NL + lz : -1;
  };
  auto store = [&](int pos, const float4& p, int at, float uw) {
    if (WITH_NRM) {
      S.rec0[pos] = p;
      S.src[pos] = at;
    } else {
      const int gid = __float_as_int(p.w);
      const bool own = gid >= h.id_base && gid < h.id_base + h.n_own;
      int m = __float_as_int(uw) & 0xff;
      if (VS == 8) m = (m & 1) | ((m & 2) << 7) | ((m & 4) << 14) | ((m & 8) << 21);
      m |= own ? 0 : (int)0x80000000;
      S.rec0[pos] = make_float4(p.x, p.y, p.z, __int_as_float(m));
      S.gid[pos] = gid;
    }
  };
  auto scan_cells = [&]() {
    if (tid < 64) {                                  // exclusive scan of the NCELL counters by one wave
      constexpr int PER = (NCELL + 63) / 64;
      int sum = 0;
      for (int k = 0; k < PER; ++k) { const int c = tid * PER + k; sum += c < NCELL ? S.ccur[c] : 0; }
      int ex = iso_wave_incl_scan(sum) - sum;
      for (int k = 0; k < PER; ++k) {
        const int c = tid * PER + k;
        if (c < NCELL) { const int v = S.ccur[c]; S.cstart[c] = ex; S.ccur[c] = ex; ex += v; }
      }
      if (tid == 63) S.cstart[NCELL] = ex;
    }
  };
  if (total_raw <= BK_THREADS * BK_RAW) {
    int idx[BK_RAW], cell[BK_RAW];
    float4 p[BK_RAW];
    // slot k of this WAVE holds records only when live(k) -- a scalar test, so the empty slots (on a surface half of the
    // eight) cost a branch instead of their share of ~1000 predicated-off instructions per wave
    const int wbase = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    auto live = [&](int k) { return wbase + k * BK_THREADS < total_raw; };
#pragma unroll
    for (int k = 0; k < BK_RAW; ++k) {
      idx[k] = -1; cell[k] = -1;
      p[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live(k)) {
        const int j = tid + k * BK_THREADS;
        idx[k] = j < total_raw ? index_of(j) : -1;
      }
    }
#pragma unroll
    for (int k = 0; k < BK_RAW; ++k)
      if (live(k)) p[k] = idx[k] >= 0 ? rec0[idx[k]] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < BK_RAW; ++k) {
      if (live(k)) {
        cell[k] = idx[k] >= 0 ? cell_of(p[k]) : -1;
        if (cell[k] >= 0) atomicAdd(&S.ccur[cell[k]], 1);
      }
    }
    __syncthreads();
    scan_cells();
    __syncthreads();
    if (S.cstart[NCELL] > CAP) return -1;
    const float* __restrict__ rec1w = reinterpret_cast<const float*>(rec1) + 3;     // the payload word of a second record
    float uw[BK_RAW];
#pragma unroll
    for (int k = 0; k < BK_RAW; ++k) {               // (bandwidth kernel) the payload words of the accepted candidates, all in flight
      uw[k] = 0.f;
      if (!WITH_NRM && live(k)) uw[k] = cell[k] >= 0 ? rec1w[4 * (int64_t)idx[k]] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < BK_RAW; ++k)
      if (live(k)) { if (cell[k] >= 0) store(atomicAdd(&S.ccur[cell[k]], 1), p[k], idx[k], uw[k]); }
  } else {                                           // very dense neighbourhood: two passes over global memory
    for (int j = tid; j < total_raw; j += BK_THREADS) {
      const int c = cell_of(rec0[index_of(j)]);
      if (c >= 0) atomicAdd(&S.ccur[c], 1);
    }
    __syncthreads();
    scan_cells();
    __syncthreads();
    if (S.cstart[NCELL] > CAP) return -1;
    for (int j = tid; j < total_raw; j += BK_THREADS) {
      const int i = index_of(j);
      const float4 p = rec0[i];
      const int c = cell_of(p);
      if (c >= 0) store(atomicAdd(&S.ccur[c], 1), p, i, WITH_NRM ? 0.f : rec1[i].w);
    }
  }
  constexpr int NQ = St::NQRUN, QA = 4 * SUB;        // the brick's own (sub-)cells: QA x QA contiguous z-runs of QA
  int qlen = 0;
  if (tid < NQ) {
    // (cstart is final since the scan; ccur is being advanced by the scatter above; qt: opaque as rt above)
    int qt = tid;
    asm volatile("" : "+v"(qt));
    const int c = ((SUB + qt / QA) * NL + (SUB + qt % QA)) * NL + SUB;
    S.qbeg[qt] = S.cstart[c];
    qlen = S.cstart[c + QA] - S.cstart[c];
  }
  if (tid < 64) {                                    // exclusive prefix of the run lengths (NQ <= 64: one wave)
    const int inc = iso_wave_incl_scan(qlen);
    if (tid < NQ) S.qpre[tid + 1] = inc;
    if (tid == 0) S.qpre[0] = 0;
  }
  __syncthreads();
  return S.cstart[NCELL];
}

template <bool WITH_NRM, int SUB, int CAP>
__device__ __forceinline__ int query_slot(const BrickStage<WITH_NRM, SUB, CAP>& S, int t) {
  int lo = 0, hi = BrickStage<WITH_NRM, SUB, CAP>::NQRUN;         // the run r with qpre[r] <= t < qpre[r + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (S.qpre[mid] <= t) lo = mid; else hi = mid;
  }
  return S.qbeg[lo] + (t - S.qpre[lo]);
}

// The 3x3x3 fine cells around local cell (lx,ly,lz) = nine contiguous slot ranges of the staged block, walked as ONE
// loop per lane: two candidates per trip (both LDS reads issued before either is used; v0 / v1 say which of them
// exist), and a lane that reaches the end of a range moves on to the next one in the same trip -- the bounds of the
// range after that are requested then and are there when they are needed.  The first form ran the nine ranges as nine
// loops: a wave then pays the LONGEST of its lanes' ranges nine times (measured: ~125 trips per wave for ~46 per
// lane); as one loop it pays the longest total.  An empty range costs its lane one idle trip.
template <bool WITH_NRM, int CAP, class Body>
__device__ __forceinline__ void walk_candidates(const BrickStage<WITH_NRM, 1, CAP>& S, int lx, int ly, int lz, Body&& body) {
  constexpr int NL = BrickStage<WITH_NRM, 1, CAP>::NL;
  int cell = ((lx - 1) * NL + (ly - 1)) * NL + (lz - 1);            // range r: cell + (r / 3) NL^2 + (r % 3) NL, three cells
  int i = S.cstart[cell], e = S.cstart[cell + 3];
  cell += NL;
  int ni = S.cstart[cell], ne = S.cstart[cell + 3];                 // range 1
  int run = 0, m = 1;                                               // m = (index of the prefetched range) % 3
  while (run < 9) {
    const bool v0 = i < e, v1 = i + 1 < e;
    const int i0 = v0 ? i : 0, i1 = v1 ? i + 1 : i0;
    float4 c0 = S.rec0[i0];
    float4 c1 = S.rec0[i1];
    // both records are consumed HERE as far as the compiler can tell: left to itself it sinks the second read into the
    // `v1` branch and its payload word into the distance test (three LDS round trips per trip, one after the other)
    asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z), "+v"(c0.w), "+v"(c1.x), "+v"(c1.y), "+v"(c1.z), "+v"(c1.w));
    body(c0, c1, v0, v1);
    i += 2;
    if (i >= e) {
      ++run;
      i = ni; e = ne;
      m = m == 2 ? 0 : m + 1;
      cell += m == 0 ? NL * NL - 2 * NL : NL;
      if (run < 8) { ni = S.cstart[cell]; ne = S.cstart[cell + 3]; }
    }
  }
}

// The same nine ranges NEAREST FIRST, with an early exit: the column of the query's own cell, then the columns on the side
// of the cell the query lies on (sx, sy = +-1), the far side last.  done() is asked at the end of every range; a lane that
// is done leaves the loop (the wave pays the longest of its lanes' walks).  The bandwidth kernel's counting pass only has
// to find SEVEN renderable neighbours within 0.01 per view -- in a dense cloud the first or second column holds them, so
// most of the ~9 ranges are never read (k_brick_h 163 -> see DESIGN.md 3.2).
template <bool WITH_NRM, int CAP, class Body, class Done>
__device__ __forceinline__ void walk_candidates_near_first(const BrickStage<WITH_NRM, 1, CAP>& S, int lx, int ly, int lz,
                                                           int sx, int sy, Body&& body, Done&& done) {
  constexpr int NL = BrickStage<WITH_NRM, 1, CAP>::NL;
  // step k visits column (a_k sx, b_k sy): a = 0 1 0 1 -1 0 -1 1 -1, b = 0 0 1 1 0 -1 1 -1 -1 (stored + 1, two bits each)
  constexpr unsigned KA = 1u | 2u << 2 | 1u << 4 | 2u << 6 | 0u << 8 | 1u << 10 | 0u << 12 | 2u << 14 | 0u << 16;
  constexpr unsigned KB = 1u | 1u << 2 | 2u << 4 | 2u << 6 | 1u << 8 | 0u << 10 | 2u << 12 | 0u << 14 | 0u << 16;
  const int base = (lx * NL + ly) * NL + (lz - 1);
  const int dxs = sx * NL * NL, dys = sy * NL;
  auto cell_at = [&](int k) {
    const int a = (int)((KA >> (2 * k)) & 3u) - 1, b = (int)((KB >> (2 * k)) & 3u) - 1;
    return base + a * dxs + b * dys;
  };
  int i = S.cstart[base], e = S.cstart[base + 3];
  int c = cell_at(1);
  int ni = S.cstart[c], ne = S.cstart[c + 3];
  int run = 0;
  while (run < 9) {
    const bool v0 = i < e, v1 = i + 1 < e;
    const int i0 = v0 ? i : 0, i1 = v1 ? i + 1 : i0;
    float4 c0 = S.rec0[i0];
    float4 c1 = S.rec0[i1];
    asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z), "+v"(c0.w), "+v"(c1.x), "+v"(c1.y), "+v"(c1.z), "+v"(c1.w));
    body(c0, c1, v0, v1);
    i += 2;
    if (i >= e) {
      ++run;
      if (done()) run = 9;
      i = ni; e = ne;
      if (run < 8) { c = cell_at(run + 1); ni = S.cstart[c]; ne = S.cstart[c + 3]; }
    }
  }
}

// SUB = 2: the NW x NW x NW window of half cells whose first cell is (wx, wy, wz) = NW^2 contiguous slot ranges of NW
// half cells each (NW = 6: the 3 x 3 x 3 fine cells around its cell; the query's own 4 x 4 x 4 window takes
// walk_window_flat); same two-candidates-per-trip protocol.
template <int NW, bool WITH_NRM, class Body>
__device__ __forceinline__ void walk_window(const BrickStage<WITH_NRM, 2>& S, int wx, int wy, int wz, Body&& body) {
  constexpr int NL = BrickStage<WITH_NRM, 2>::NL;
  auto cell0 = [&](int c) { return ((wx + c / NW) * NL + (wy + c % NW)) * NL + wz; };
  int a = S.cstart[cell0(0)], e = S.cstart[cell0(0) + NW];
  for (int c = 0; c < NW * NW; ++c) {
    int na = 0, ne = 0;
    if (c < NW * NW - 1) { na = S.cstart[cell0(c + 1)]; ne = S.cstart[cell0(c + 1) + NW]; }
    for (int i = a; i < e; i += 2) {
      const bool two = i + 1 < e;
      const int i1 = two ? i + 1 : i;
      const float4 c0 = S.rec0[i];
      const float4 c1 = S.rec0[i1];
      body(c0, i, c1, i1, true, two);
    }
    a = na; e = ne;
  }
}

// The same window as ONE loop per lane (see walk_candidates): a wave pays the longest total of its lanes' NW^2 ranges
// instead of the longest range NW^2 times.  body(c0, i0, c1, i1, v0, v1): v0 / v1 say which of the two records exist.
template <int NW, bool WITH_NRM, class Body>
__device__ __forceinline__ void walk_window_flat(const BrickStage<WITH_NRM, 2>& S, int wx, int wy, int wz, Body&& body) {
  constexpr int NL = BrickStage<WITH_NRM, 2>::NL;
  int cell = (wx * NL + wy) * NL + wz;                              // range c: cell + (c / NW) NL^2 + (c % NW) NL, NW half cells
  int i = S.cstart[cell], e = S.cstart[cell + NW];
  cell += NL;
  int ni = S.cstart[cell], ne = S.cstart[cell + NW];                // range 1
  int run = 0, m = 1;                                               // m = (index of the prefetched range) % NW
  while (run < NW * NW) {
    const bool v0 = i < e, v1 = i + 1 < e;
    const int i0 = v0 ? i : 0, i1 = v1 ? i + 1 : i0;
    const float4 c0 = S.rec0[i0];
    const float4 c1 = S.rec0[i1];
    body(c0, i0, c1, i1, v0, v1);
    i += 2;
    if (i >= e) {
      ++run;
      i = ni; e = ne;
      m = m == NW - 1 ? 0 : m + 1;
      cell += m == 0 ? NL * NL - (NW - 1) * NL : NL;
      if (run < NW * NW - 1) { ni = S.cstart[cell]; ne = S.cstart[cell + NW]; }
    }
  }
}

// a brick whose neighbourhood does not fit LDS: its own points go to the tail kernel
__device__ void brick_to_tail(const BrickHdr& h, const int32_t* __restrict__ off, const float4* __restrict__ rec0, int b,
                              int32_t* __restrict__ tail, int32_t* __restrict__ counters, int tail_slot, int per_query) {
  for (int i = off[BK_CPB * b] + threadIdx.x; i < off[BK_CPB * (b + 1)]; i += BK_THREADS) {
    const int gid = __float_as_int(rec0[i].w);
    if (gid >= h.id_base && gid < h.id_base + h.n_own) {
      const int at = atomicAdd(&counters[tail_slot], per_query);
      for (int v = 0; v < per_query; ++v) tail[at + v] = per_query > 1 ? (gid - h.id_base) * 8 + v : gid - h.id_base;
    }
  }
  if (threadIdx.x == 0) atomicAdd(&counters[2], 1);
}

// Which brick of the list a workgroup takes.  Workgroup i of a launch runs on XCD i % 8 (tools/probes/simd_map.hip prints
// it), and each XCD has its own L2: dealt out in list order, the eight neighbours of a brick -- whose records it stages,
// and whose queries write into the same cache lines of the row-ordered outputs -- sit in eight different L2s.  With
// kXcdChunks = 8 the list (x-major brick order: consecutive entries are neighbours along z, then y) is cut into eight
// contiguous chunks and XCD k walks chunk k.
constexpr int kXcdChunks = 8;
__device__ __forceinline__ int bk_xcd_span(int n_list) {
  return kXcdChunks * ((n_list + kXcdChunks - 1) / kXcdChunks);
}
__device__ __forceinline__ int bk_xcd_item(int lj, int n_list) {
  const int chunk = (n_list + kXcdChunks - 1) / kXcdChunks;
  return (lj % kXcdChunks) * chunk + lj / kXcdChunks;
}

// Grids of the two fused kernels: a workgroup per brick or two, handed out by the dispatcher as CUs free up.  Bricks differ
// widely in cost (points per brick, lanes with an open view) and a persistent grid that strides over the list ends with a
// long tail: measured on the cfg-3a cycle, k_brick_h 241 us at 2048 workgroups, 211 at 3840, 186 at 10240 (flat beyond);
// k_brick_resample 291 / 287 / 270 us at 1024 / 2048 / >= 4096.  A workgroup past the end of the list reads one counter
// and leaves.
static int brick_grid(int64_t n_own, int cap) {
  int64_t g = n_own / 48;
  if (g < 1024) g = 1024;
  if (g > cap) g = cap;
  return (int)g;
}

}  // namespace
