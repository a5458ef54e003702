// The K front-most entries of a pixel in its thread's registers, on the total order (z, id): the list of the splat
// raster (splat_raster.hip, splat_bins.hip; with the carried q column) and of the mesh raster (mesh_raster.hip; z and id
// only).  The order is total, so a list does not depend on the order in which its candidates arrive.
#pragma once
#include <float.h>

namespace {

template <int KMAX, bool WITH_Q = true>
struct KBest {
  float z[KMAX];
  float q[WITH_Q ? KMAX : 0];    // between z and id, empty without q: moving it (last, or into a base class: first)
                                 // changed the register order of k_raster / k_raster_merge or of k_mesh_raster
  int id[KMAX];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      z[j] = FLT_MAX;
      if (WITH_Q) q[j] = -1.f;
      id[j] = 0x7fffffff;
    }
  }
  __device__ __forceinline__ bool live(int j) const { return z[j] < FLT_MAX; }
  // The branchy swap chain: orders by float compares, so it takes any depth (a -0 included).  k_fine_bins' form.
  __device__ __forceinline__ void push(float cz, int ci, float cq, int K) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < K && (cz < z[j] || (cz == z[j] && ci < id[j]))) {
        float tz = z[j], tq = q[j]; int ti = id[j];
        z[j] = cz; q[j] = cq; id[j] = ci;
        cz = tz; cq = tq; ci = ti;
      }
    }
  }
  // The masked insertion.  Depths here are >= +0 and never NaN (binning drops z < 0 and NaN, the caller adds +0.0f so
  // that -0 is +0): their float order is the order of their bit patterns as unsigned integers, and (z, id) "less" is
  // three integer compares whose masks go straight into the selects -- no tie pass, no ballot, no boolean arrays in
  // vector registers (the first form, a tie pass and v_med3_f32 per level, compiled to ~200 instructions per insertion;
  // knock-outs of round 5: the insertions were 98 of the raster kernel's 207 us).
  //   push_masked(z, id, K)          (z, id) alone: the caller recomputes what else it needs for the K survivors at the end
  //   push_masked<true>(z, id, K, q)  q carried along, for lists that are merged (k_raster_merge): entries come from
  //                                   lists made by the first form
  // One body and no push_zi / push_q wrappers around it: a wrapper is one more inlining level, and that changed the
  // instruction schedule of k_raster<4, true> and k_raster_merge<8..32> (tools/kernel_isa_diff.py).
  template <bool CARRY_Q = false>
  __device__ __forceinline__ void push_masked(float cz, int ci, int K, float cq = 0.f) {
    const unsigned cu = __float_as_uint(cz);
    bool m[KMAX];
    const bool full = K == KMAX;                        // (uniform: the usual case drops the slot test)
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      const unsigned zu = __float_as_uint(z[j]);
      // `|` and `&`, not `||` and `&&`: three compares and two mask operations, no branch per level
      m[j] = (full | (j < K)) & ((cu < zu) | ((cu == zu) & (ci < id[j])));
    }
#pragma unroll
    for (int j = KMAX - 1; j >= 1; --j) {
      z[j] = m[j - 1] ? z[j - 1] : (m[j] ? cz : z[j]);
      if (CARRY_Q) q[j] = m[j - 1] ? q[j - 1] : (m[j] ? cq : q[j]);
      id[j] = m[j - 1] ? id[j - 1] : (m[j] ? ci : id[j]);
    }
    z[0] = m[0] ? cz : z[0];
    if (CARRY_Q) q[0] = m[0] ? cq : q[0];
    id[0] = m[0] ? ci : id[0];
  }
};

template <int KMAX>
using PixK = KBest<KMAX, true>;

}  // namespace
