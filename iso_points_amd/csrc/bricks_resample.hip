// The fused resample step on the brick grid (bricks.h; built by bricks.hip): the FRNN K+1 query and the tangent-plane
// repulsion in one kernel, neighbour data staged in LDS (bricks_stage.h), and its one-wave tail (bricks_walk.h).
//
// Reference semantics
//   neighbour tree  : UniformProjection._create_tree, DSS/models/levelset_sampling.py:110-140
//                     (r = sqrt(diag/P) * knn_k, K+1 self-inclusive FRNN query, column 0 dropped)
//   repulsion       : UniformProjection.resample, levelset_sampling.py:254-284
// The stand-alone iso_frnn_* entry points (frnn.hip) stay the general API (any K, any radius,
// foreign query sets); these kernels are the hot path of the iso-point cycle.  Results are the same
// exact "K nearest within r, ties to the lower index" lists; tests pin one against the other.
//
// Selection without per-candidate branches: a lane keeps the M = K + 3 smallest 32-bit keys
// (d2 bits with the low 10 bits replaced by the candidate's LDS slot) in a sorted register list,
// one v_med3_u32 per slot and candidate.  Truncated keys order like d2 up to 2^-13 relative, so the
// exact (d2, id) order is restored afterwards on the M survivors; the list is certified complete
// when the first key beyond the K-th differs from it in the kept bits (else: tail kernel).
#include <type_traits>
#include "bricks_stage.h"
#include "bricks_walk.h"
#include "topk.h"

#pragma clang fp contract(off)

namespace {

// ---- the repulsion of one point given its sorted neighbours (levelset_sampling.py:268-284) ------
struct Repulse {
  float px, py, pz, inv_sigma;
  float sw = 0.f, mx = 0.f, my = 0.f, mz = 0.f;
  // (ux, uy, uz): the neighbour's UNIT normal -- F.normalize of levelset_sampling.py:258 is applied once per point when
  // the records are written (bk_unit_normal in the scatter kernels) instead of once per (query, neighbour) pair here:
  // the same operations on the same operands, so the same bits, and three IEEE divisions + a square root fewer per pair
  __device__ __forceinline__ void add(float qx, float qy, float qz, float ux, float uy, float uz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const float w = expf(-d2 * inv_sigma);
    const float dn = (dx * ux + dy * uy) + dz * uz;
    const float tx = dx - dn * ux, ty = dy - dn * uy, tz = dz - dn * uz;
    sw += w;
    mx += w * tx; my += w * ty; mz += w * tz;
  }
  __device__ __forceinline__ void finish(float* __restrict__ o) const {
    const float dens = sw + 1.0f;
    const float den = iso_eps_denom(sw, 1.0e-17f);
    o[0] = px + dens * mx / den;
    o[1] = py + dens * my / den;
    o[2] = pz + dens * mz / den;
  }
};

// ---- fused resample step -------------------------------------------------------------------------
// K = knn_k + 1 (self included), M = list length (>= K + 1).
template <int M>
__global__ __launch_bounds__(BK_THREADS, 4) void k_brick_resample(
    const BrickHdr* __restrict__ hp, const int32_t* __restrict__ off, const int32_t* __restrict__ list,
    const float4* __restrict__ rec0, const float4* __restrict__ rec1, int K, float* __restrict__ out,
    int64_t* __restrict__ idx_out, float* __restrict__ d2_out, int32_t* __restrict__ tail,
    int32_t* __restrict__ counters) {
  __shared__ BrickStage<true, 2> S;
  __shared__ int s_unc[BK_THREADS], s_nunc;
  const BrickHdr h = *hp;
  const int n_list = counters[0];
  for (int lj = blockIdx.x; lj < bk_xcd_span(n_list); lj += gridDim.x) {
    const int li = bk_xcd_item(lj, n_list);
    if (li >= n_list) continue;
    const int b = list[li];
    BrickGeo g;
    if (threadIdx.x == 0) s_nunc = 0;                  // (stage_brick starts with a barrier)
    const int C = stage_brick<true, 1, 2>(S, h, off, rec0, rec1, b, g);
    if (C < 0) { brick_to_tail(h, off, rec0, b, tail, counters, 1, 1); continue; }
    const int nq = S.qpre[BrickStage<true, 2>::NQRUN];
    // One query, start to finish.  WIDE = false: the 4 x 4 x 4 window of half cells picked by the half of its own half
    // cell the query lies in: two below and one above on the axes where it lies in the lower half, one below and two
    // above otherwise -- every point within (2 - m) half cells is inside, m = the largest distance of the query from
    // the middle plane of its half cell over the axes (0 <= m <= 1/2): 0.75 .. 1 fine cells.  WIDE = true: the 3 x 3 x 3
    // fine cells around its cell (6^3 half cells; everything within one fine cell), for the few queries the first
    // window cannot certify.  Returns false when the result could not be certified (nothing is written then).
    // The wide pass runs with a list two entries longer when M = K + 1: a query whose (K + 1)-th key ties with its K-th
    // fails the list test whatever the window, and would otherwise end in the tail kernel (a wave per query).
    auto one_query = [&](int pos, auto wide_tag) -> bool {
      constexpr bool WIDE = decltype(wide_tag)::value;
      constexpr int ML = (WIDE && M == 10) ? 12 : M;
      const float4 q = S.rec0[pos];
      const int gid = __float_as_int(q.w);
      int wx, wy, wz;
      float mfrac = 0.f;
      {
        auto win = [&](float pc, float mn, int nf, int o) {
          const float t2 = ((pc - mn) * h.inv_f) * 2.0f;
          int sc = (int)floorf(t2);
          sc = sc < 0 ? 0 : (sc >= 2 * nf ? 2 * nf - 1 : sc);
          if (WIDE) return 2 * (sc >> 1) - 2 * o - 2;                 // the fine cell below the query's
          const float fr = t2 - (float)sc;
          const bool low = fr < 0.5f;
          mfrac = fmaxf(mfrac, low ? fr : 1.0f - fr);
          return sc - 2 * o - (low ? 2 : 1);
        };
        wx = win(q.x, h.mn[0], h.nf[0], g.ox);
        wy = win(q.y, h.mn[1], h.nf[1], g.oy);
        wz = win(q.z, h.mn[2], h.nf[2], g.oz);
      }
      float gq2 = h.g2;                                               // (0.999 f)^2: the wide window
      if (!WIDE) { const float gq = (2.0f - mfrac) * 0.5f; gq2 = (gq * gq) * h.g2; }
      unsigned key[ML];
#pragma unroll
      for (int j = 0; j < ML; ++j) key[j] = 0xffffffffu;
      auto visit = [&](const float4& c0, int i0, const float4& c1, int i1, bool v0, bool v1) {
        const float da = bk_d2(q.x, q.y, q.z, c0.x, c0.y, c0.z);
        const float db = bk_d2(q.x, q.y, q.z, c1.x, c1.y, c1.z);
        const unsigned ka = v0 ? ((__float_as_uint(da) & ~1023u) | (unsigned)i0) : 0xffffffffu;
        const unsigned kb = v1 ? ((__float_as_uint(db) & ~1023u) | (unsigned)i1) : 0xffffffffu;
#pragma unroll
        for (int j = ML - 1; j >= 1; --j) key[j] = bk_med3u(key[j - 1], ka, key[j]);
        key[0] = min(key[0], ka);
#pragma unroll
        for (int j = ML - 1; j >= 1; --j) key[j] = bk_med3u(key[j - 1], kb, key[j]);
        key[0] = min(key[0], kb);
      };
      if (WIDE) walk_window<6>(S, wx, wy, wz, visit);
      else walk_window_flat<4>(S, wx, wy, wz, visit);
      // exact (d2, id) order of the survivors
      float d[ML];
      int id[ML], ps[ML];
#pragma unroll
      for (int j = 0; j < ML; ++j) {
        const bool valid = key[j] != 0xffffffffu;
        ps[j] = valid ? (int)(key[j] & 1023u) : pos;
        const float4 c = S.rec0[ps[j]];
        const float d2 = bk_d2(q.x, q.y, q.z, c.x, c.y, c.z);
        const bool ok = valid && d2 < h.r2;
        d[j] = ok ? d2 : FLT_MAX;
        id[j] = ok ? __float_as_int(c.w) : 0x7fffffff;
      }
      bool swapped;
      do {
        swapped = false;
#pragma unroll
        for (int j = 0; j + 1 < ML; ++j) {
          if (pair_lt(d[j + 1], id[j + 1], d[j], id[j])) {
            const float td = d[j]; d[j] = d[j + 1]; d[j + 1] = td;
            const int ti = id[j]; id[j] = id[j + 1]; id[j + 1] = ti;
            const int tp = ps[j]; ps[j] = ps[j + 1]; ps[j + 1] = tp;
            swapped = true;
          }
        }
      } while (swapped);
      unsigned kK = 0xffffffffu;
      float dK = FLT_MAX;
#pragma unroll
      for (int j = 0; j < ML; ++j) if (j == K - 1) { kK = key[j]; dK = d[j]; }
      const bool cert_list = key[ML - 1] == 0xffffffffu || (key[ML - 1] >> 10) > (kK >> 10);
      const bool cert_geo = gq2 >= h.r2 || (dK < FLT_MAX && dK <= gq2);
      if (!(cert_list && cert_geo)) return false;
      const int row = gid - h.id_base;
      Repulse R;
      R.px = q.x; R.py = q.y; R.pz = q.z; R.inv_sigma = h.inv_sigma;
      // the normals of the K - 1 neighbours come from the brick-sorted array (four requests in flight)
#pragma unroll
      for (int j0 = 1; j0 < ML; j0 += 4) {
        float4 u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = j0 + k;
          u[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (j < ML && j < K && d[j < ML ? j : 0] < FLT_MAX) u[k] = rec1[S.src[ps[j < ML ? j : 0]]];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = j0 + k;
          if (j < ML && j < K && d[j < ML ? j : 0] < FLT_MAX) {
            const float4 c = S.rec0[ps[j < ML ? j : 0]];
            R.add(c.x, c.y, c.z, u[k].x, u[k].y, u[k].z);
          }
        }
      }
      R.finish(out + (int64_t)row * 3);
      if (idx_out) {
#pragma unroll
        for (int j = 1; j < ML; ++j)
          if (j < K) {
            idx_out[(int64_t)row * (K - 1) + j - 1] = d[j] < FLT_MAX ? (int64_t)id[j] : (int64_t)-1;
            if (d2_out) d2_out[(int64_t)row * (K - 1) + j - 1] = d[j] < FLT_MAX ? d[j] : -1.0f;
          }
      }
      return true;
    };
    auto to_tail = [&](int pos) { tail[atomicAdd(&counters[1], 1)] = __float_as_int(S.rec0[pos].w) - h.id_base; };
    for (int t = threadIdx.x; t < nq; t += BK_THREADS) {
      const int pos = query_slot(S, t);
      const int gid = __float_as_int(S.rec0[pos].w);
      if (gid < h.id_base || gid >= h.id_base + h.n_own) continue;          // imported halo point
      if (!one_query(pos, std::false_type())) {
        // (~0.1 % of the queries of a uniform cloud) queued for the wide window: done by densely packed lanes below
        const int at = atomicAdd(&s_nunc, 1);
        if (at < BK_THREADS) s_unc[at] = pos; else to_tail(pos);
      }
    }
    __syncthreads();
    const int n_unc = min(s_nunc, BK_THREADS);
    for (int u = threadIdx.x; u < n_unc; u += BK_THREADS) {
      const int pos = s_unc[u];
      if (!one_query(pos, std::true_type())) to_tail(pos);                   // beyond one fine cell: rings of bricks
    }
  }
}

// ---- the tail: one wave per query, rings of bricks (bricks_walk.h) --------------------------------
// A lane's list is TopK<KMAX, true> (topk.h): the K smallest (d, id) with the sorted position of the record alongside.
// K rounds of a wave-wide arg-min over the lanes' list heads.  emit(k, d, id, at) is called with
// wave-uniform arguments for k = 0..K-1 (d == FLT_MAX: no such neighbour); returns the K-th distance.
template <int KMAX, class Emit>
__device__ __forceinline__ float wave_merge3(const TopK<KMAX, true>& best, int K, Emit&& emit) {
  int head = 0;
  float kth = FLT_MAX;
  for (int k = 0; k < K; ++k) {
    float hd = FLT_MAX;
    int hi = 0x7fffffff, ha = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) if (j == head) { hd = best.d[j]; hi = best.id[j]; ha = best.at[j]; }
    float md = hd;
    int mi = hi, ma = ha;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_xor(md, o);
      const int oi = __shfl_xor(mi, o), oa = __shfl_xor(ma, o);
      if (pair_lt(od, oi, md, mi)) { md = od; mi = oi; ma = oa; }
    }
    if (hd == md && hi == mi && md < FLT_MAX) ++head;
    if (k == K - 1) kth = md;
    emit(k, md, mi, ma);
  }
  return kth;
}

template <int KMAX>
__global__ __launch_bounds__(64) void k_brick_resample_tail(
    const BrickHdr* __restrict__ hp, const int32_t* __restrict__ off, const float4* __restrict__ rec0,
    const float4* __restrict__ rec1, const float* __restrict__ pts, int K, float* __restrict__ out,
    int64_t* __restrict__ idx_out, float* __restrict__ d2_out, const int32_t* __restrict__ tail,
    const int32_t* __restrict__ counters) {
  const BrickHdr h = *hp;
  const int lane = threadIdx.x;
  const int count = counters[1];
  const float B = 4.0f * h.f;
  const int rho_max = max(h.nb[0], max(h.nb[1], h.nb[2]));
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int row = tail[w];
    const float qx = pts[(int64_t)row * 3], qy = pts[(int64_t)row * 3 + 1], qz = pts[(int64_t)row * 3 + 2];
    const int qbx = bk_fine(qx, h.mn[0], h.inv_f, h.nf[0]) >> 2;
    const int qby = bk_fine(qy, h.mn[1], h.inv_f, h.nf[1]) >> 2;
    const int qbz = bk_fine(qz, h.mn[2], h.inv_f, h.nf[2]) >> 2;
    TopK<KMAX, true> best;
    best.init();
    float wd = FLT_MAX;
    int wi = 0x7fffffff;
    int found = 0;
    const WalkGeo geo = {qx, qy, qz, h.mn[0], h.mn[1], h.mn[2], B};
    float kth_seen = FLT_MAX;                               // K-th distance of the wave at the last ring end
    // a lane that holds K records within wd proves that the K-th distance of the query is <= wd
    auto far2 = [&]() {
      float m = wd;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
      return fminf(h.r2, fminf(m, kth_seen));
    };
    for (int rho = 0; rho <= rho_max; ++rho) {
      bk_walk_ring(rho, qbx, qby, qbz, h.nb[0], h.nb[1], h.nb[2], off, lane, geo, [&](int i) { return rec0[i]; },
                   [&](int i, const float4& c) {
        const float d2 = bk_d2(qx, qy, qz, c.x, c.y, c.z);
        if (d2 < h.r2) {
          if (found < KMAX) ++found;
          const int ci = __float_as_int(c.w);
          if (pair_lt(d2, ci, wd, wi)) {
            best.push(d2, ci, K, i);
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if (j == K - 1) { wd = best.d[j]; wi = best.id[j]; }
          }
        }
      }, far2, far2);
      if (rho >= 1) {
        const float gg = (float)rho * B * 0.999f;
        if (gg >= h.r) break;
        int tot = found;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        if (tot >= K) {
          const float kth = wave_merge3<KMAX>(best, K, [](int, float, int, int) {});
          kth_seen = fminf(kth_seen, kth);
          if (kth < FLT_MAX && kth <= gg * gg) break;
        }
      }
    }
    Repulse R;
    R.px = qx; R.py = qy; R.pz = qz; R.inv_sigma = h.inv_sigma;
    const float kthf = wave_merge3<KMAX>(best, K, [&](int k, float md, int mi, int ma) {
      if (k == 0) return;                                  // column 0 is dropped (levelset_sampling.py:136-138)
      if (md < FLT_MAX) {
        const float4 c = rec0[ma];
        const float4 u = rec1[ma];
        R.add(c.x, c.y, c.z, u.x, u.y, u.z);
      }
      if (idx_out && lane == 0) {
        idx_out[(int64_t)row * (K - 1) + k - 1] = md < FLT_MAX ? (int64_t)mi : (int64_t)-1;
        if (d2_out) d2_out[(int64_t)row * (K - 1) + k - 1] = md < FLT_MAX ? md : -1.0f;
      }
    });
    if (lane == 0) {
      R.finish(out + (int64_t)row * 3);
      const float need = kthf < FLT_MAX ? sqrtf(kthf) : h.r;         // how far this query had to look
      if (qx - need < h.x_lo || qx + need >= h.x_hi) atomicAdd(const_cast<int32_t*>(&counters[6]), 1);
    }
  }
}

}  // namespace

// ================================================================================================
static int resample_grid(int64_t n_own) { return brick_grid(n_own, 8192); }

extern "C" int iso_resample_fused(void* workspace, int64_t n_max, const float* points, int64_t n_own,
                                  int k_plus_one, float* points_out, int64_t* idx_out, float* d2_out,
                                  void* stream) {
  ISO_REQUIRE(workspace && n_own >= 0 && n_max >= n_own, ISO_ERR_INVALID, "iso_resample_fused: bad arguments");
  ISO_REQUIRE(k_plus_one >= 2 && k_plus_one <= 13, ISO_ERR_UNSUPPORTED,
              "iso_resample_fused: K + 1 must be in [2,13], got %d", k_plus_one);
  if (n_own == 0) return ISO_OK;
  ISO_REQUIRE(points && points_out && points != points_out, ISO_ERR_INVALID, "iso_resample_fused: null / aliased pointer");
  const BrickWs w = bricks_carve(workspace, n_max);
  hipStream_t s = (hipStream_t)stream;
  const int K = k_plus_one;
#define ISO_RS(MM)                                                                                           \
  hipLaunchKernelGGL(k_brick_resample<MM>, dim3(resample_grid(n_own)), dim3(BK_THREADS), 0, s, w.hdr, w.off, w.list, \
                     w.rec0, w.rec1, K, points_out, idx_out, d2_out, w.tail, w.counters)
  // (list length K + 1 is the shortest that can certify: the 10-entry list of the default K = 9 fails the list test for
  // ~0.1 % of the queries -- they take the wide window -- and saves two of twelve insertion steps per candidate)
  if (K <= 5) ISO_RS(8);
  else if (K == 9) ISO_RS(10);
  else if (K <= 9) ISO_RS(12);
  else ISO_RS(16);
#undef ISO_RS
  int tb = (int)(n_own < 4096 ? n_own : 4096);
  hipLaunchKernelGGL(k_brick_resample_tail<16>, dim3(tb), dim3(64), 0, s, w.hdr, w.off, w.rec0, w.rec1, points, K,
                     points_out, idx_out, d2_out, w.tail, w.counters);
  ISO_CHECK_LAUNCH("iso_resample_fused");
  return ISO_OK;
}
