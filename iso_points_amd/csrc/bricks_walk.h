// The walk of the tail kernels of the brick grid (k_brick_resample_tail in bricks_resample.hip, k_brick_h_tail in
// bricks_h.hip): a query that its brick's LDS block could not certify searches level 1 of bricks.h, the brick-sorted
// records in global memory, ring by ring around its own brick.  Private to csrc/.
#pragma once
#include "bricks.h"

#pragma clang fp contract(off)

namespace {

// ---- rings of bricks around a query (tail kernels: one wave per query) ---------------------------
// The record ranges of up to 64 columns of bricks are fetched by 64 lanes at once (a ring then costs one
// global-memory latency for its bounds instead of one per column); the records of those columns are one index
// space split over the lanes.  bound() (wave-uniform, asked once per 64 columns) is the squared distance beyond
// which a record cannot matter any more -- the radius, or the K-th distance found so far: bricks whose box lies
// farther than that from the query are dropped before their records are read (a stray point of the SIREN level
// set 0.15 off the surface would otherwise scan the whole shell of bricks that reaches the surface anywhere).
struct WalkGeo { float qx, qy, qz, mnx, mny, mnz, B; };
constexpr int kWalkItems = 8;   // record loads a lane keeps in flight (4 until round 3: a stray query's few thousand records were a
                                // chain of ~40 batch latencies)

// bk_walk_shell: the bricks at Chebyshev distance rin + 1 .. rho from the query's brick (rin = rho - 1: one ring;
// rin = -1: the whole cube).  A query that found too little in rings 0 and 1 -- a stray point -- takes all the remaining
// rings up to the radius as ONE shell: a ring is a chain of two dependent global latencies (brick bounds, records), five
// rings one after the other were the critical path of the bandwidth tail kernel (150 us in the SIREN cycle for a few
// thousand stray queries).
// part / nparts: the trips of a batch of columns are dealt out to nparts waves that walk the same shell (each of them
// fetches the bounds and forms the prefix sums itself); 0 / 1 = one wave does everything.
// Two bounds.  bound(), asked once per 64 columns, decides which runs enter the index space the trips are dealt from: with
// nparts > 1 it must return the SAME value in every cooperating wave (else the waves would number the records
// differently and visit some twice and others never).  local(), asked before every trip, is the wave's own, sharper
// knowledge (its lanes' K-th distance so far): runs whose box lies beyond it stay in the index space but are not loaded.
template <class Fetch, class Body, class Bound, class Local>
__device__ __forceinline__ void bk_walk_shell(int rin, int rho, int qbx, int qby, int qbz, int nbx, int nby, int nbz,
                                              const int32_t* __restrict__ off, int lane, const WalkGeo& G,
                                              Fetch&& fetch, Body&& body, Bound&& bound, Local&& local,
                                              int part = 0, int nparts = 1) {
  const int x0 = max(qbx - rho, 0), x1 = min(qbx + rho, nbx - 1);
  const int y0 = max(qby - rho, 0), y1 = min(qby + rho, nby - 1);
  if (x0 > x1 || y0 > y1) return;
  const int ny = y1 - y0 + 1, ncols = (x1 - x0 + 1) * ny;
  for (int c0 = 0; c0 < ncols; c0 += 64) {
    int s0 = 0, e0 = 0, s1 = 0, e1 = 0;                  // this lane's column: one z-run (edge) or two caps
    float dm0 = FLT_MAX, dm1 = FLT_MAX;                  // squared distance from the query to the boxes of the runs
    const int col = c0 + lane;
    const float far2 = bound();
    // squared distance from the query to bricks [b0, b1] of one axis, shortened by a margin that covers the
    // rounding of the brick assignment (so that "farther than far2" is never claimed wrongly)
    auto gap = [&](float q, float mn, int b0, int b1) {
      const float lo = mn + (float)b0 * G.B, hi = mn + (float)(b1 + 1) * G.B;
      return fmaxf(0.f, fmaxf(lo - q, q - hi) - 1e-3f * G.B);
    };
    if (col < ncols) {
      const int x = x0 + col / ny, y = y0 + col % ny;
      const bool edge = x < qbx - rin || x > qbx + rin || y < qby - rin || y > qby + rin;   // outside the inner square
      const int cb = (x * nby + y) * nbz;
      const float gx = gap(G.qx, G.mnx, x, x), gy = gap(G.qy, G.mny, y, y);
      const float gxy2 = gx * gx + gy * gy;
      auto box2 = [&](int za, int zb) { const float gz = gap(G.qz, G.mnz, za, zb); return gxy2 + gz * gz; };
      // the bricks of the column that a ball of far2 around the query can reach (same margin as gap(): never too few)
      const float dz = sqrtf(fmaxf(far2 - gxy2, 0.f)) + 1e-3f * G.B;
      const int zc0 = (int)fmaxf(floorf((G.qz - dz - G.mnz) / G.B), 0.f);
      const int zc1 = (int)fminf(floorf((G.qz + dz - G.mnz) / G.B), (float)(nbz - 1));
      if (edge) {
        const int za = max(max(qbz - rho, 0), zc0), zb = min(min(qbz + rho, nbz - 1), zc1);
        if (za <= zb && (dm0 = box2(za, zb)) <= far2) { s0 = off[BK_CPB * (cb + za)]; e0 = off[BK_CPB * (cb + zb + 1)]; }
      } else {                                            // two caps: below and above the inner cube
        const int a0 = max(max(qbz - rho, 0), zc0), a1 = min(qbz - rin - 1, zc1);
        const int b0 = max(qbz + rin + 1, zc0), b1 = min(min(qbz + rho, nbz - 1), zc1);
        if (a0 <= a1 && (dm0 = box2(a0, a1)) <= far2) { s0 = off[BK_CPB * (cb + a0)]; e0 = off[BK_CPB * (cb + a1 + 1)]; }
        if (b0 <= b1 && (dm1 = box2(b0, b1)) <= far2) { s1 = off[BK_CPB * (cb + b0)]; e1 = off[BK_CPB * (cb + b1 + 1)]; }
      }
    }
    // a lane finds the column of its item in the prefix sums of the column lengths
    const int len0 = e0 - s0, len = len0 + (e1 - s1);
    int inc = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    const int ex = inc - len, total = __shfl(inc, 63);
    constexpr int NU = kWalkItems;                           // items per lane and trip: their loads overlap
    for (int j0 = part * 64 * NU; j0 < total; j0 += nparts * 64 * NU) {
      const float near2 = local();
      const int live = (dm0 <= near2 ? 1 : 0) | (dm1 <= near2 ? 2 : 0);
      int at[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int j = j0 + u * 64 + lane;
        int c = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {         // the last column whose prefix is <= j holds item j
          const int cand = c + step;
          const int v = __shfl(ex, cand & 63);
          if (cand < 64 && v <= j) c = cand;
        }
        const int cs0 = __shfl(s0, c), cl0 = __shfl(len0, c), cs1 = __shfl(s1, c), cex = __shfl(ex, c);
        const int clive = __shfl(live, c);
        const int r = j - cex;
        at[u] = j < total ? (r < cl0 ? cs0 + r : cs1 + (r - cl0)) : -1;
        if (!(clive & (r < cl0 ? 1 : 2))) at[u] = -1;
      }
      decltype(fetch(0)) rec[NU];                            // loads first (no control flow in between), then the work
#pragma unroll
      for (int u = 0; u < NU; ++u) rec[u] = fetch(at[u] >= 0 ? at[u] : 0);
#pragma unroll
      for (int u = 0; u < NU; ++u)
        if (at[u] >= 0) body(at[u], rec[u]);
    }
  }
}

template <class Fetch, class Body, class Bound, class Local>
__device__ __forceinline__ void bk_walk_ring(int rho, int qbx, int qby, int qbz, int nbx, int nby, int nbz,
                                             const int32_t* __restrict__ off, int lane, const WalkGeo& G,
                                             Fetch&& fetch, Body&& body, Bound&& bound, Local&& local,
                                             int part = 0, int nparts = 1) {
  bk_walk_shell(rho - 1, rho, qbx, qby, qbz, nbx, nby, nbz, off, lane, G, fetch, body, bound, local, part, nparts);
}

// (The two tail kernels open with the same lines -- query position, its brick, B, rho_max, the WalkGeo.  Stated once here
// as a struct filled from (h, pts, row), all three tail kernels compiled to different machine code: the text stays.)

}  // namespace
