// The fused per-view splat bandwidth h on the brick grid (bricks.h; built by bricks.hip): the K = 7 query of every
// view's visible cloud in ONE pass over the whole cloud, candidates staged in LDS (bricks_stage.h), and its four- or
// eight-wave tail (bricks_walk.h).
//
// Reference semantics
//   splat bandwidth : SurfaceSplatting._get_per_point_info, DSS/core/rasterizer.py:367-386
//                     (K = 7 self query of the filtered view cloud, h = clamp(max d2 / 2, 5e-5, 0.01))
// The view mask the kernels read is the set-up stage's (k_view_mask in splat.hip, or the follow part of a projection:
// follow.h).  The stand-alone path (iso_frnn_* + iso_splat_vrk_h) stays the general API; tests pin one against the other.
#include "bricks_stage.h"
#include "bricks_walk.h"

#pragma clang fp contract(off)

namespace {

// ---- fused splat bandwidth -----------------------------------------------------------------------
// h of a point in view v from the sorted 7 smallest d2 among the view's points within r (self
// included): the stand-alone path takes max(dists[1..6]) of a -1-padded row (iso_splat_vrk_h).
__device__ __forceinline__ float h_from_list(const float* d /*7 ascending, FLT_MAX = none*/, bool small_cloud) {
  float m = -FLT_MAX;
#pragma unroll
  for (int k = 1; k < 7; ++k) {
    const float v = small_cloud ? 1e-3f : (d[k] < FLT_MAX ? d[k] : -1.0f);
    m = fmaxf(m, v);
  }
  return fminf(fmaxf(0.5f * m, 5e-5f), 0.01f);
}

// (five waves per SIMD: 277 -> 257 us with a persistent grid; six with a workgroup per brick, see kHWgs and h_grid();
// the resample kernel (bricks_resample.hip) is bound by its instruction count and gains nothing)
constexpr int kHWgs = 6;     // workgroups per CU (5 / 6 / 7: 189 / 181 / 196 us with a workgroup per brick)
template <int NV>
__global__ __launch_bounds__(BK_THREADS, NV <= 4 ? kHWgs : 4) void k_brick_h(
    const BrickHdr* __restrict__ hp, const int32_t* __restrict__ off, const int32_t* __restrict__ list,
    const float4* __restrict__ rec0, const float4* __restrict__ rec1, const int32_t* __restrict__ view_total,
    int n_views, float* __restrict__ h_out /*(n_views, n_own)*/, int32_t* __restrict__ tail,
    int32_t* __restrict__ counters) {
  __shared__ BrickStage<false, 1, BK_CAP> S;
  const BrickHdr h = *hp;
  const int n_list = counters[0];
  bool small_cloud[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) small_cloud[v] = v < n_views && view_total[v] < 7;
  // 0.5 d2 <= 5e-5 (the lower clamp of h) <=> d2 <= kT: seven such points settle h without their order
  const float kT = 2.0f * 5e-5f;
  const float t2 = fminf(kT, h.r2 > 0.f ? __uint_as_float(__float_as_uint(h.r2) - 1u) : 0.f);   // and d2 < r2
  for (int lj = blockIdx.x; lj < bk_xcd_span(n_list); lj += gridDim.x) {
    const int li = bk_xcd_item(lj, n_list);
    if (li >= n_list) continue;
    const int b = list[li];
    BrickGeo g;
    constexpr int VS = NV <= 4 ? 8 : 1;                 // staged view masks: one byte per view when they fit a word
    const int C = stage_brick<false, VS, 1, BK_CAP>(S, h, off, rec0, rec1, b, g);
    if (C < 0) { brick_to_tail(h, off, rec0, b, tail, counters, 3, 8); continue; }
    const int nq = S.qpre[16];
    for (int t0 = 0; t0 < nq; t0 += BK_THREADS) {
      const int t = t0 + threadIdx.x;
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      int qmask = 0, lx = 1, ly = 1, lz = 1, row = 0, sx = 1, sy = 1;
      if (t < nq) {
        const int pos = query_slot(S, t);
        q = S.rec0[pos];
        qmask = __float_as_int(q.w);
        if (qmask < 0) qmask = 0;                                    // imported halo point: not a query
        row = S.gid[pos] - h.id_base;
        const int fx = bk_fine(q.x, h.mn[0], h.inv_f, h.nf[0]), fy = bk_fine(q.y, h.mn[1], h.inv_f, h.nf[1]);
        lx = fx - g.ox;
        ly = fy - g.oy;
        lz = bk_fine(q.z, h.mn[2], h.inv_f, h.nf[2]) - g.oz;
        // the half of its cell the query lies in (only the ORDER of the walk depends on it)
        sx = ((q.x - h.mn[0]) * h.inv_f - (float)fx) >= 0.5f ? 1 : -1;
        sy = ((q.y - h.mn[1]) * h.inv_f - (float)fy) >= 0.5f ? 1 : -1;
      }
      // pass 1: renderable neighbours within kT per view, counted until every view of the query has seven (cnt[v] is
      // the full count only where it stays below seven -- all the rest of the kernel asks)
      int cnt[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) cnt[v] = 0;
      if (VS == 8 && C <= 255) {                                     // (workgroup-uniform) byte counters cannot overflow
        unsigned acc = 0;
        const unsigned need = ((unsigned)qmask & 0x01010101u) << 7;
        if (qmask)
          walk_candidates_near_first(S, lx, ly, lz, sx, sy, [&](const float4& c0, const float4& c1, bool v0, bool v1) {
            const float da = bk_d2(q.x, q.y, q.z, c0.x, c0.y, c0.z);
            const float db = bk_d2(q.x, q.y, q.z, c1.x, c1.y, c1.z);
            const unsigned ma = (v0 && da <= t2) ? (__float_as_uint(c0.w) & 0x01010101u) : 0u;
            const unsigned mb = (v1 && db <= t2) ? (__float_as_uint(c1.w) & 0x01010101u) : 0u;
            acc += ma + mb;
          }, [&]() {      // bit 7 of every byte: that counter is >= 7 (no carry between bytes: 0x7f + 0x79 < 0x100)
            const unsigned ge7 = (((acc & 0x7f7f7f7fu) + 0x79797979u) | acc) & 0x80808080u;
            return (ge7 & need) == need;
          });
#pragma unroll
        for (int v = 0; v < NV; ++v) cnt[v] = (int)((acc >> (8 * (v & 3))) & 0xffu);
      } else if (qmask)
        walk_candidates_near_first(S, lx, ly, lz, sx, sy, [&](const float4& c0, const float4& c1, bool v0, bool v1) {
          const float da = bk_d2(q.x, q.y, q.z, c0.x, c0.y, c0.z);
          const float db = bk_d2(q.x, q.y, q.z, c1.x, c1.y, c1.z);
          const int ma = (v0 && da <= t2) ? __float_as_int(c0.w) : 0;
          const int mb = (v1 && db <= t2) ? __float_as_int(c1.w) : 0;
#pragma unroll
          for (int v = 0; v < NV; ++v) cnt[v] += ((ma >> (VS * v)) & 1) + ((mb >> (VS * v)) & 1);
        }, [&]() {
          bool all = true;
#pragma unroll
          for (int v = 0; v < NV; ++v) all = all && (!((qmask >> (VS * v)) & 1) || cnt[v] >= 7);
          return all;
        });
      bool open_ = false;
#pragma unroll
      for (int v = 0; v < NV; ++v) open_ = open_ || (((qmask >> (VS * v)) & 1) && !small_cloud[v] && cnt[v] < 7);
      // pass 2 (only the lanes with an open view; rare away from the terminator of a dense cloud):
      // the 7 smallest d2 per view
      float d[NV][7];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int j = 0; j < 7; ++j) d[v][j] = FLT_MAX;
      if (open_)
        walk_candidates(S, lx, ly, lz, [&](const float4& c0, const float4& c1, bool v0, bool v1) {
          float da = bk_d2(q.x, q.y, q.z, c0.x, c0.y, c0.z);
          float db = bk_d2(q.x, q.y, q.z, c1.x, c1.y, c1.z);
          da = (v0 && da < h.r2) ? da : FLT_MAX;
          db = (v1 && db < h.r2) ? db : FLT_MAX;
          const int ma = __float_as_int(c0.w), mb = __float_as_int(c1.w);
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const float ka = (ma >> (VS * v)) & 1 ? da : FLT_MAX;
            const float kb = (mb >> (VS * v)) & 1 ? db : FLT_MAX;
#pragma unroll
            for (int j = 6; j >= 1; --j) d[v][j] = __builtin_amdgcn_fmed3f(d[v][j - 1], ka, d[v][j]);
            d[v][0] = fminf(d[v][0], ka);
#pragma unroll
            for (int j = 6; j >= 1; --j) d[v][j] = __builtin_amdgcn_fmed3f(d[v][j - 1], kb, d[v][j]);
            d[v][0] = fminf(d[v][0], kb);
          }
        });
      if (qmask) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          if (v < n_views && ((qmask >> (VS * v)) & 1)) {
            float hv;
            bool cert = true;
            if (small_cloud[v]) hv = fminf(fmaxf(0.5f * 1e-3f, 5e-5f), 0.01f);
            else if (cnt[v] >= 7) hv = 5e-5f;
            else {
              cert = h.g_covers_r || (d[v][6] < FLT_MAX && d[v][6] <= h.g2);
              hv = h_from_list(d[v], false);
            }
            if (cert) h_out[(int64_t)v * h.n_own + row] = hv;
            else tail[atomicAdd(&counters[3], 1)] = row * 8 + v;
          }
        }
      }
    }
  }
}

template <int KMAX>
struct TopF {
  float d[KMAX];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) d[j] = FLT_MAX;
  }
  __device__ __forceinline__ void push(float k) {
#pragma unroll
    for (int j = KMAX - 1; j >= 1; --j) d[j] = __builtin_amdgcn_fmed3f(d[j - 1], k, d[j]);
    d[0] = fminf(d[0], k);
  }
};

// the 7 smallest values of the union of the lanes' sorted lists, wave-uniform
__device__ __forceinline__ void wave_merge_f7(const TopF<7>& best, float* out7) {
  int head = 0;
  for (int k = 0; k < 7; ++k) {
    float hd = FLT_MAX;
#pragma unroll
    for (int j = 0; j < 7; ++j) if (j == head) hd = best.d[j];
    float md = hd;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) md = fminf(md, __shfl_xor(md, o));
    // exactly one of the lanes holding the minimum pops (the lowest lane)
    const unsigned long long holders = __ballot(hd == md && md < FLT_MAX);
    if (holders && (int)(__ffsll((long long)holders) - 1) == (int)(threadIdx.x & 63)) ++head;
    out7[k] = md;
  }
}

// What the clamp of h_from_list makes of the search: 0.5 d2 >= 0.01 for every d2 >= kHSat, so a list that holds ANY
// distance in [kHSat, r2) among its entries 1..6 gives h = 0.01 whatever the others are.  The tail search therefore keeps
// exact distances only below kHSat and a flag "some renderable point lies in [kHSat, r2)": once the flag is up nothing
// beyond sqrt(kHSat) = 0.141 can change the result (r = 0.2 in the reference's settings: half the shell's volume).
// (0.5f * 0.02f == 0.01f exactly: the two constants share their mantissa.)
constexpr float kHSat = 0.02f;

// One WORKGROUP of four waves per uncertified (query, view): a stray point of the SIREN level set finds nothing nearby and
// scans the whole shell of bricks up to the radius -- ~10 k records, a chain of ~20 batches of loads for one wave, and the
// longest such chain is what the launch takes (120 us in the SIREN cycle however many workgroups share the few thousand
// entries).  The four waves deal the batches out among themselves and pool their seven smallest distances through LDS at
// the ring ends.
constexpr int kHTailWaves = 4;   // waves per workgroup of k_brick_h_tail (eight below kTailWideBelow points)
// (kTailWaves <= 9: the pooled selection runs in one wave.  Eight waves instead of four: a rank's share of eight 51 -> 40 us,
// the 1 M-point cycle 72-75 -> 83-86 -- the launcher takes eight for clouds below kTailWideBelow points.)
constexpr int64_t kTailWideBelow = 300000;
template <int kTailWaves>
__global__ __launch_bounds__(64 * kTailWaves) void k_brick_h_tail(
    const BrickHdr* __restrict__ hp, const int32_t* __restrict__ off, const float4* __restrict__ rec0,
    const float4* __restrict__ rec1, const float* __restrict__ pts, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ view_total, int n_views, float* __restrict__ h_out,
    const int32_t* __restrict__ tail, const int32_t* __restrict__ counters) {
  __shared__ float s_m7[2][kTailWaves][8];     // [.][.][7]: the wave saw a distance in [kHSat, r2)
  const BrickHdr h = *hp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int count = counters[3];
  const float B = 4.0f * h.f;
  const int rho_max = max(h.nb[0], max(h.nb[1], h.nb[2]));
  int pool_buf = 0;
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int row = tail[w] >> 3, v = tail[w] & 7;
    if (v >= n_views || !((mask[row] >> v) & 1)) continue;           // (a whole overflowing brick was queued)
    const float qx = pts[(int64_t)row * 3], qy = pts[(int64_t)row * 3 + 1], qz = pts[(int64_t)row * 3 + 2];
    const int qbx = bk_fine(qx, h.mn[0], h.inv_f, h.nf[0]) >> 2;
    const int qby = bk_fine(qy, h.mn[1], h.inv_f, h.nf[1]) >> 2;
    const int qbz = bk_fine(qz, h.mn[2], h.inv_f, h.nf[2]) >> 2;
    const bool small_cloud = view_total[v] < 7;
    TopF<7> best;
    best.init();
    float m7[7];
    const WalkGeo geo = {qx, qy, qz, h.mn[0], h.mn[1], h.mn[2], B};
    float kth_seen = FLT_MAX;
    bool sat = false;                                       // this lane met a distance in [kHSat, r2)
    bool sat_any = false;                                   // ... some lane of the workgroup did (as far as this wave knows)
    bool sat_all = false;                                   // sat_any as of the last pool(): the same in every wave
    auto far2 = [&]() {                                     // a lane's own 7th distance bounds the query's (this wave's view)
      float m = best.d[6];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
      sat_any = sat_any || __any(sat);
      return fminf(sat_any ? kHSat : h.r2, fminf(m, kth_seen));
    };
    auto far2_all = [&]() { return fminf(sat_all ? kHSat : h.r2, kth_seen); };    // what all four waves agree on
    // the seven smallest distances of the workgroup: every wave's seven through LDS, then one more selection
    auto pool = [&]() {
      wave_merge_f7(best, m7);
      sat_any = sat_any || __any(sat);
      if (lane < 8) {
        float mine = m7[0];
#pragma unroll
        for (int k = 1; k < 7; ++k) mine = lane == k ? m7[k] : mine;
        s_m7[pool_buf][wave][lane] = lane == 7 ? (sat_any ? 1.f : 0.f) : mine;
      }
      __syncthreads();
      TopF<7> all;
      all.init();
      if (lane < 7 * kTailWaves) all.push(s_m7[pool_buf][lane / 7][lane % 7]);
      wave_merge_f7(all, m7);
#pragma unroll
      for (int k = 0; k < kTailWaves; ++k) sat_any = sat_any || s_m7[pool_buf][k][7] != 0.f;
      sat_all = sat_any;
      pool_buf ^= 1;                                        // (the next pool writes the other buffer: no second barrier)
    };
    auto fetch = [&](int i) { float4 c = rec0[i]; c.w = rec1[i].w; return c; };          // position + view mask
    auto visit = [&](int, const float4& c) {
      if (!((__float_as_int(c.w) >> v) & 1)) return;
      const float d2 = bk_d2(qx, qy, qz, c.x, c.y, c.z);
      if (d2 < kHSat) { if (d2 < h.r2) best.push(d2); }
      else if (d2 < h.r2) sat = true;
    };
    // rings 0 and 1 one after the other (most queries end there); a query that is still open -- a stray point -- takes
    // every remaining ring up to the radius as one shell (bk_walk_shell)
    int rho_r = 1;                                          // first ring whose guarantee rho * B covers the radius
    while (rho_r < rho_max && (float)rho_r * B * 0.999f < h.r) ++rho_r;
    for (int rho = 0; rho <= min(1, rho_max); ++rho) {
      bk_walk_ring(rho, qbx, qby, qbz, h.nb[0], h.nb[1], h.nb[2], off, lane, geo, fetch, visit, far2_all, far2, wave, kTailWaves);
      if (rho >= 1) {
        const float gg = (float)rho * B * 0.999f;
        if (gg >= h.r) { rho_r = 1; break; }
        pool();
        kth_seen = fminf(kth_seen, m7[6]);
        if (m7[6] < FLT_MAX && m7[6] <= gg * gg) { rho_r = 1; break; }
        if (sat_any && kHSat <= gg * gg) { rho_r = 1; break; }          // everything below kHSat was seen
      }
    }
    if (rho_r > 1)
      bk_walk_shell(1, rho_r, qbx, qby, qbz, h.nb[0], h.nb[1], h.nb[2], off, lane, geo, fetch, visit, far2_all, far2, wave, kTailWaves);
    pool();
    if (threadIdx.x == 0) {
      // fewer than seven below kHSat and something in [kHSat, r2): entry 1..6 of the full list holds a value >= kHSat
      const bool saturated = m7[6] == FLT_MAX && sat_any && !small_cloud;
      h_out[(int64_t)v * h.n_own + row] = saturated ? 0.01f : h_from_list(m7, small_cloud);
      const float need = m7[6] < FLT_MAX ? sqrtf(m7[6]) : (sat_any ? fminf(sqrtf(kHSat), h.r) : h.r);
      if (!small_cloud && (qx - need < h.x_lo || qx + need >= h.x_hi)) atomicAdd(const_cast<int32_t*>(&counters[6]), 1);
    }
  }
}

}  // namespace

// ================================================================================================
static int h_grid(int64_t n_own) { return brick_grid(n_own, 10240); }

extern "C" int iso_splat_h_fused(void* workspace, int64_t n_max, const float* points, const int32_t* mask,
                                 int64_t n_own, const int32_t* view_total, int n_views, float* h_out,
                                 void* stream) {
  ISO_REQUIRE(workspace && n_own >= 0 && n_max >= n_own, ISO_ERR_INVALID, "iso_splat_h_fused: bad arguments");
  ISO_REQUIRE(n_views >= 1 && n_views <= 8, ISO_ERR_UNSUPPORTED, "iso_splat_h_fused: 1..8 views per call");
  if (n_own == 0) return ISO_OK;
  ISO_REQUIRE(points && mask && view_total && h_out, ISO_ERR_INVALID, "iso_splat_h_fused: null pointer");
  const BrickWs w = bricks_carve(workspace, n_max);
  hipStream_t s = (hipStream_t)stream;
#define ISO_H(NV)                                                                                            \
  hipLaunchKernelGGL(k_brick_h<NV>, dim3(h_grid(n_own)), dim3(BK_THREADS), 0, s, w.hdr, w.off, w.list, w.rec0, \
                     w.rec1, view_total, n_views, h_out, w.tail, w.counters)
  if (n_views <= 1) ISO_H(1);
  else if (n_views <= 2) ISO_H(2);
  else if (n_views <= 4) ISO_H(4);
  else ISO_H(8);
#undef ISO_H
  if (n_own < kTailWideBelow)
    hipLaunchKernelGGL((k_brick_h_tail<2 * kHTailWaves>), dim3(4096), dim3(64 * 2 * kHTailWaves), 0, s, w.hdr, w.off, w.rec0, w.rec1, points, mask, view_total,
                     n_views, h_out, w.tail, w.counters);
  else
    hipLaunchKernelGGL((k_brick_h_tail<kHTailWaves>), dim3(4096), dim3(64 * kHTailWaves), 0, s, w.hdr, w.off, w.rec0, w.rec1, points, mask, view_total,
                     n_views, h_out, w.tail, w.counters);
  ISO_CHECK_LAUNCH("iso_splat_h_fused");
  return ISO_OK;
}
