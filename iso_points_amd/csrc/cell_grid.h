// The walk over the uniform cell grid of frnn.hip, stated once for the kernels that search it (k_query, k_query_tail,
// k_cham_nearest, k_pf_nearest).  Device code only, private to csrc/.
//
// A cloud's points are sorted by cell (x-major, z fastest), so a run of cells of one (x, y) column is one contiguous
// range of (x, y, z, original index) records.  A query walks Chebyshev shells of cells around its own cell: shells 0 and
// 1 together as the nine z-runs of the 3x3x3 block, every further shell rho column by column -- an edge column
// (|x - cx| = rho or |y - cy| = rho) is one z-run, an interior column its two cap cells.  After shell rho every point
// within ring_reach(rho, cell) of the query has been seen.  The visitors below clamp to the grid and hand each run to
// `visit(i0, i1)` as a record range.  Candidates are ordered by (d2, index) with d2 = rec_d2(), so a result does not
// depend on the order of visits, nor on which kernel or lane served the query.
//
// Who finishes a query its lane leaves open: a search for the single nearest target (k_cham_nearest, k_pf_nearest) runs
// nearest_walk() below, which owns both phases -- the lane's own shells, then the lane's whole wave, one open query after
// the other, inside the same launch.  Such a kernel supplies how a record range is scored, when a query is closed and
// how the wave gets at another lane's query, nothing else.  The K-best list of k_query and its hand-off of open queries to
// k_query_tail through a second launch stay with frnn.hip.
#pragma once
#include <float.h>
#include "iso_common.h"
#include "topk.h"      // pair_lt, wave_argmin: the (d2, index) order

#pragma clang fp contract(off)

namespace {

constexpr int kRingCap = 2;   // shells a lane walks alone beyond its first; an open query then goes to a whole wave

struct Grid3 {
  float mnx, mny, mnz, delta, cell;   // origin, cells per unit length, cell size
  int rx, ry, rz, total;
};

__device__ __forceinline__ Grid3 grid3_load(const float* __restrict__ params, int n) {
  const float* gp = params + n * ISO_GRID3_PARAMS;
  Grid3 g;
  g.mnx = gp[0]; g.mny = gp[1]; g.mnz = gp[2]; g.delta = gp[3];
  g.rx = (int)gp[4]; g.ry = (int)gp[5]; g.rz = (int)gp[6]; g.total = (int)gp[7];
  g.cell = 1.0f / g.delta;
  return g;
}

// the unclamped integer cell of a query (it may lie outside the grid), the first shell that touches the grid box
// (rho0: the distance in cells from the query's cell to the box; shells below it are empty) and the shell beyond
// which no cell exists (span)
struct QueryCell { int cx, cy, cz, rho0, span; };

__device__ __forceinline__ QueryCell query_cell(const Grid3& g, float qx, float qy, float qz) {
  const float lim = 1.0e6f;
  QueryCell c;
  c.cx = (int)fminf(fmaxf(floorf((qx - g.mnx) * g.delta), -lim), lim);
  c.cy = (int)fminf(fmaxf(floorf((qy - g.mny) * g.delta), -lim), lim);
  c.cz = (int)fminf(fmaxf(floorf((qz - g.mnz) * g.delta), -lim), lim);
  const int gapx = c.cx < 0 ? -c.cx : (c.cx >= g.rx ? c.cx - g.rx + 1 : 0);
  const int gapy = c.cy < 0 ? -c.cy : (c.cy >= g.ry ? c.cy - g.ry + 1 : 0);
  const int gapz = c.cz < 0 ? -c.cz : (c.cz >= g.rz ? c.cz - g.rz + 1 : 0);
  c.rho0 = max(gapx, max(gapy, gapz));
  c.span = max(g.rx, max(g.ry, g.rz)) + c.rho0;
  return c;
}

// every point within this distance of the query lies in the shells 0..rho of its cell
__device__ __forceinline__ float ring_reach(int rho, float cell) { return (float)rho * cell * 0.999f; }

// the records of cells za..zb (inside the grid) of column (x, y); off = the cloud's cell offsets, len = its length
template <class Visit>
__device__ __forceinline__ void visit_run(const Grid3& g, const int32_t* __restrict__ off, int64_t len, int x, int y,
                                          int za, int zb, Visit&& visit) {
  const int c0 = (x * g.ry + y) * g.rz + za, c1 = (x * g.ry + y) * g.rz + zb;
  visit((int64_t)off[c0], (c1 + 1 < g.total) ? (int64_t)off[c1 + 1] : len);
}

// shells 0 and 1 together: the nine z-runs of the 3x3x3 block around a cell inside the grid
template <class Visit>
__device__ __forceinline__ void visit_block27(const Grid3& g, const int32_t* __restrict__ off, int64_t len,
                                              const QueryCell& c, Visit&& visit) {
  const int za = max(c.cz - 1, 0), zb = min(c.cz + 1, g.rz - 1);
  for (int x = max(c.cx - 1, 0); x <= min(c.cx + 1, g.rx - 1); ++x)
    for (int y = max(c.cy - 1, 0); y <= min(c.cy + 1, g.ry - 1); ++y) visit_run(g, off, len, x, y, za, zb, visit);
}

// the cells of column (x, y) that belong to shell rho
template <class Visit>
__device__ __forceinline__ void visit_shell_column(const Grid3& g, const int32_t* __restrict__ off, int64_t len,
                                                   const QueryCell& c, int rho, int x, int y, Visit&& visit) {
  const bool edge = (x == c.cx - rho) || (x == c.cx + rho) || (y == c.cy - rho) || (y == c.cy + rho);
  const int nseg = (edge || rho == 0) ? 1 : 2;
  for (int sgm = 0; sgm < nseg; ++sgm) {
    int za, zb;
    if (edge) { za = c.cz - rho; zb = c.cz + rho; }
    else if (sgm == 0) { za = c.cz - rho; zb = c.cz - rho; }
    else { za = c.cz + rho; zb = c.cz + rho; }
    za = max(za, 0); zb = min(zb, g.rz - 1);
    if (za > zb) continue;
    visit_run(g, off, len, x, y, za, zb, visit);
  }
}

// all columns of shell rho, by one lane
template <class Visit>
__device__ __forceinline__ void visit_shell_lane(const Grid3& g, const int32_t* __restrict__ off, int64_t len,
                                                 const QueryCell& c, int rho, Visit&& visit) {
  const int x0 = max(c.cx - rho, 0), x1 = min(c.cx + rho, g.rx - 1);
  const int y0 = max(c.cy - rho, 0), y1 = min(c.cy + rho, g.ry - 1);
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) visit_shell_column(g, off, len, c, rho, x, y, visit);
}

// all columns of shell rho, split over the 64 lanes of a wave (c and rho wave-uniform): lane l takes columns l, l + 64, ...
template <class Visit>
__device__ __forceinline__ void visit_shell_wave(const Grid3& g, const int32_t* __restrict__ off, int64_t len,
                                                 const QueryCell& c, int rho, int lane, Visit&& visit) {
  const int x0 = max(c.cx - rho, 0), x1 = min(c.cx + rho, g.rx - 1);
  const int y0 = max(c.cy - rho, 0), y1 = min(c.cy + rho, g.ry - 1);
  if (x0 <= x1 && y0 <= y1) {
    const int ny = y1 - y0 + 1;
    const int ncols = (x1 - x0 + 1) * ny;
    for (int col = lane; col < ncols; col += 64) visit_shell_column(g, off, len, c, rho, x0 + col / ny, y0 + col % ny, visit);
  }
}

// squared distance from the query to a record: the expression the oracle evaluates (contraction off)
__device__ __forceinline__ float rec_d2(float qx, float qy, float qz, const float4& rec) {
  const float dx = qx - rec.x, dy = qy - rec.y, dz = qz - rec.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// cand(d2, original index) for every record of [i0, i1), two per trip: two independent 16-B loads in flight per lane
template <class Cand>
__device__ __forceinline__ void scan_run2(const float4* __restrict__ s4, int64_t i0, int64_t i1, float qx, float qy,
                                          float qz, Cand&& cand) {
  for (int64_t i = i0; i < i1; i += 2) {
    const bool two = i + 1 < i1;
    const float4 ca = s4[i];
    const float4 cb = s4[two ? i + 1 : i];
    cand(rec_d2(qx, qy, qz, ca), __float_as_int(ca.w));
    if (two) cand(rec_d2(qx, qy, qz, cb), __float_as_int(cb.w));
  }
}

// ---- the nearest target of one query per lane, (d2, index) smallest ---------------------------------------------------
// The lane walks the 3x3x3 block and up to kRingCap further shells alone; a query still open then (an isolated point, a
// query far from the targets, a stop rule that needs a long reach) is finished by the whole wave, one open query after the
// other: one slow lane would otherwise hold its wave for thousands of dependent loads.  The kernel supplies
//   score(q, i0, i1, bd, bi) : the records [i0, i1) against query q, folded into the pair (bd, bi)
//   closed(q, bd, rho)       : nothing beyond shell rho (>= 1) can beat bd
//   wave_query(src, q)       : q = lane src's query, the same value in every lane of the wave
// and starts from bd = FLT_MAX, bi = INT_MAX; the result is left in the owning lane, bd = FLT_MAX without a target.

// where a lane left its query: its cell, the next shell to walk, and whether anything is left to walk
struct WalkState { QueryCell c; int rho_next; bool open; };

// the lane's own shells of the query `own` at p.  A function of its own: written into nearest_walk, k_pf_nearest<1> needs
// 131 instead of 127 VGPRs and loses a wave
template <class Q, class Score, class Closed>
__device__ __forceinline__ WalkState nearest_lane_phase(const Grid3& g, const int32_t* __restrict__ off, int64_t len,
                                                        const Q& own, float px, float py, float pz, Score&& score,
                                                        Closed&& closed, float& bd, int& bi) {
  WalkState w;
  w.c = query_cell(g, px, py, pz);
  const int rho_stop = min(w.c.span, w.c.rho0 + kRingCap);
  auto scan = [&](int64_t i0, int64_t i1) { score(own, i0, i1, bd, bi); };
  w.open = true;
  int rho = w.c.rho0;
  if (w.c.rho0 == 0 && rho_stop >= 1) {
    visit_block27(g, off, len, w.c, scan);
    if (closed(own, bd, 1)) w.open = false;
    rho = 2;
  }
  for (; rho <= rho_stop && w.open; ++rho) {
    visit_shell_lane(g, off, len, w.c, rho, scan);
    if (rho >= 1 && closed(own, bd, rho)) w.open = false;
  }
  w.rho_next = rho;
  if (w.rho_next > w.c.span) w.open = false;
  return w;
}

// both phases; EVERY lane of the wave calls it, `live` says whether the lane has a query at all
template <class Q, class Score, class Closed, class WaveQuery>
__device__ __forceinline__ void nearest_walk(const Grid3& g, const int32_t* __restrict__ off, int64_t len, int lane,
                                             bool live, const Q& own, float px, float py, float pz, Score&& score,
                                             Closed&& closed, WaveQuery&& wave_query, float& bd, int& bi) {
  WalkState w = {{0, 0, 0, 0, -1}, 0, false};
  if (live) w = nearest_lane_phase(g, off, len, own, px, py, pz, score, closed, bd, bi);
  unsigned long long todo = __ballot(w.open);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    Q wq;
    wave_query(src, wq);
    QueryCell wc;
    wc.cx = __shfl(w.c.cx, src); wc.cy = __shfl(w.c.cy, src); wc.cz = __shfl(w.c.cz, src);
    wc.rho0 = __shfl(w.c.rho0, src); wc.span = __shfl(w.c.span, src);
    const int w_first = __shfl(w.rho_next, src);
    float wd = __shfl(bd, src);
    int wi = __shfl(bi, src);
    for (int rho = w_first; rho <= wc.span; ++rho) {
      visit_shell_wave(g, off, len, wc, rho, lane, [&](int64_t i0, int64_t i1) { score(wq, i0, i1, wd, wi); });
      wave_argmin(wd, wi);
      if (rho >= 1 && closed(wq, wd, rho)) break;
    }
    if (lane == src) { bd = wd; bi = wi; }
  }
}

// the records the walk reads: (x, y, z, original index as bits) per sorted point -- one 16-B load per candidate instead of
// three strided dword loads plus the index load
__global__ void k_pack_xyzi(const float* __restrict__ sorted, const int32_t* __restrict__ sorted_idx,
                            const int64_t* __restrict__ lengths, int64_t p_stride, float4* __restrict__ out) {
  const int n = blockIdx.y;
  const int64_t len = lengths ? lengths[n] : p_stride;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float* q = sorted + ((int64_t)n * p_stride + i) * 3;
    out[(int64_t)n * p_stride + i] = make_float4(q[0], q[1], q[2], __int_as_float(sorted_idx[(int64_t)n * p_stride + i]));
  }
}

inline void pack_xyzi(const float* sorted, const int32_t* sorted_idx, const int64_t* lengths, int n_clouds,
                      int64_t p_stride, float4* out, hipStream_t s) {
  if (p_stride <= 0) return;
  int gp = iso_div_up(p_stride, 256);
  if (gp > 4096) gp = 4096;
  hipLaunchKernelGGL(k_pack_xyzi, dim3(gp, n_clouds), dim3(256), 0, s, sorted, sorted_idx, lengths, p_stride, out);
}

}  // namespace
