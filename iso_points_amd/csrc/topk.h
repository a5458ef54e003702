// The K nearest candidates of a query in its lane's registers, on the total order (d2, id): the list of the cell-grid
// search (k_query, k_query_tail in frnn.hip) and, with the position of the record carried along, of the brick grid's
// resample tail (k_brick_resample_tail in bricks_resample.hip).  The order is total, so a list does not depend on the
// order in which its candidates arrive.  Device code only, private to csrc/.
#pragma once
#include <float.h>

namespace {

__device__ __forceinline__ bool pair_lt(float d1, int i1, float d2, int i2) {
  return d1 < d2 || (d1 == d2 && i1 < i2);
}

// the smallest (d, i) pair of the wave, in every lane
__device__ __forceinline__ void wave_argmin(float& d, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float od = __shfl_xor(d, o);
    const int oi = __shfl_xor(i, o);
    if (pair_lt(od, oi, d, i)) { d = od; i = oi; }
  }
}

// WITH_AT: every entry carries one more word (`at`: where its record lies), empty otherwise
template <int KMAX, bool WITH_AT = false>
struct TopK {
  float d[KMAX];
  int id[KMAX];
  int at[WITH_AT ? KMAX : 0];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      d[j] = FLT_MAX; id[j] = 0x7fffffff;
      if (WITH_AT) at[j] = 0;
    }
  }
  // keep the K smallest (d, id) pairs in ascending order
  __device__ __forceinline__ void push(float cd, int ci, int K, int ca = 0) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < K && pair_lt(cd, ci, d[j], id[j])) {
        float td = d[j]; int ti = id[j];
        d[j] = cd; id[j] = ci;
        cd = td; ci = ti;
        if (WITH_AT) { int ta = at[j]; at[j] = ca; ca = ta; }
      }
    }
  }
  __device__ __forceinline__ float worst(int K) const {
    float w = FLT_MAX;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) if (j == K - 1) w = d[j];
    return w;
  }
  __device__ __forceinline__ int worst_id(int K) const {
    int w = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) if (j == K - 1) w = id[j];
    return w;
  }
};

}  // namespace
