// The deterministic gather behind the backward passes of chamfer.hip and pfdist.hip.  Device and host code, private to
// csrc/.
//
// Every query chose one target (idx) and a target's gradient is a sum over the queries that chose it.  A counting sort on
// integer atomics (count with an arrival slot, iso_prefix_sum, fill) gives every target its list of queries in arrival
// order; the order of the SUM is fixed afterwards: gather_lane / gather_wave call f(query) in ascending query order per
// lane, and the caller adds the 64 lanes' sums by one butterfly.  No float atomics: two runs give the same bits.  What is
// summed, the scales and the write-out stay with the caller.
#pragma once
#include "iso_common.h"

namespace {

constexpr int kLightList = 8;     // targets chosen by at most this many queries are summed by their own lane
constexpr int kSortList = 1024;   // longer lists are not sorted: the wave scans the whole index row instead

// One side of a gather: per cloud a row of queries and a row of targets.  A flat packed batch is one cloud.
struct GatherView {
  const int32_t* idx;   // (clouds, q_stride): the target row a query chose; outside [0, n_t) = none
  int32_t* cnt;         // (clouds, t_stride): queries per target
  int32_t* off;         // (clouds, t_stride): where a target's list starts in its cloud's row of `list`
  int32_t* slot;        // (clouds, q_stride): a query's arrival number among those of its target
  int32_t* list;        // (clouds, q_stride)
  int64_t n_q, n_t;     // query and target rows per cloud
  int64_t q_stride, t_stride;
};
struct GatherViews { GatherView d[2]; };   // blockIdx.z picks the side, blockIdx.y the cloud

// the count pass (FILL = false: cnt and the arrival slots) and, after the prefix sum, the fill pass
template <bool FILL>
__global__ void k_gather_pass(GatherViews both) {
  const GatherView v = blockIdx.z ? both.d[1] : both.d[0];
  const int64_t qn = (int64_t)blockIdx.y * v.q_stride, tn = (int64_t)blockIdx.y * v.t_stride;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < v.n_q; j += (int64_t)gridDim.x * blockDim.x) {
    const int i = v.idx[qn + j];
    if (i < 0 || i >= v.n_t) continue;
    if (FILL) v.list[qn + v.off[tn + i] + v.slot[qn + j]] = (int32_t)j;
    else v.slot[qn + j] = atomicAdd(&v.cnt[tn + i], 1);
  }
}

// the list of target i of cloud n
__device__ __forceinline__ const int32_t* gather_list(const GatherView& v, int n, int64_t i) {
  return v.list + (int64_t)n * v.q_stride + v.off[(int64_t)n * v.t_stride + i];
}

// f(query) for the L <= kLightList entries of a list, by one lane, in ascending query order: take the smallest index above
// the last one taken, L times
template <class F>
__device__ __forceinline__ void gather_lane(const int32_t* li, int L, F&& f) {
  int last = -1;
  for (int k = 0; k < L; ++k) {
    int nxt = 0x7fffffff;
    for (int m = 0; m < L; ++m) { const int v = li[m]; if (v > last && v < nxt) nxt = v; }
    f(nxt);
    last = nxt;
  }
}

// f(query) for the L > kLightList entries of the list of target i of cloud n, by one wave that is a whole workgroup.  Up to
// kSortList entries: the list is rank-sorted into LDS (s_raw, s_sorted: kSortList ints each) and lane l takes entries l,
// l + 64, ... of the sorted list; beyond that lane l visits queries l, l + 64, ... of the cloud's index row and takes those
// that chose this target, which costs O(n_q) per such target and there are at most n_q / kSortList of them.  Either way
// every lane's calls come in ascending query order.
template <class F>
__device__ __forceinline__ void gather_wave(const GatherView& v, int n, int i, int L, int lane, int32_t* s_raw,
                                            int32_t* s_sorted, F&& f) {
  if (L <= kSortList) {
    const int32_t* li = gather_list(v, n, i);
    __syncthreads();                                   // the previous entry's readers of the LDS lists are done
    for (int m = lane; m < L; m += 64) s_raw[m] = li[m];
    __syncthreads();
    for (int m = lane; m < L; m += 64) {
      const int q = s_raw[m];
      int rank = 0;
      for (int k = 0; k < L; ++k) rank += (s_raw[k] < q) ? 1 : 0;   // query indices are distinct
      s_sorted[rank] = q;
    }
    __syncthreads();
    for (int m = lane; m < L; m += 64) f((int64_t)s_sorted[m]);
  } else {
    const int32_t* ib = v.idx + (int64_t)n * v.q_stride;
    for (int64_t j = lane; j < v.n_q; j += 64)
      if (ib[j] == i) f(j);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------
// The workspace of a gather over t_rows target rows and q_rows query rows (all clouds and sides together):
// cnt (t_rows) | heavy counters (4) | off (t_rows) | heavy (t_rows) | slot (q_rows) | list (q_rows) | 16-B aligned: the
// prefix sum's own.  cnt and the counters are zeroed together.
struct GatherWorkspace { int32_t *cnt, *heavy_count, *off, *heavy, *slot, *list; void* scan_ws; };

inline int64_t gather_ints_bytes(int64_t t_rows, int64_t q_rows) { return iso_align16(4 * (3 * t_rows + 2 * q_rows + 4)); }
inline int64_t gather_workspace_bytes(int64_t t_rows, int64_t q_rows, int64_t scan_n, int scan_batch) {
  return gather_ints_bytes(t_rows, q_rows) + iso_prefix_sum_workspace_bytes(scan_n, scan_batch) + 16;
}

inline GatherWorkspace gather_carve(void* workspace, int64_t t_rows, int64_t q_rows) {
  GatherWorkspace w;
  w.cnt = (int32_t*)workspace;
  w.heavy_count = w.cnt + t_rows;
  w.off = w.heavy_count + 4;
  w.heavy = w.off + t_rows;
  w.slot = w.heavy + t_rows;
  w.list = w.slot + q_rows;
  w.scan_ws = (char*)workspace + gather_ints_bytes(t_rows, q_rows);
  return w;
}

// zero, count, prefix sum (three launches), fill: the lists of `sides` views over `clouds` clouds each.  The target rows
// of all clouds and sides are `sides * clouds` rows of scan_n counters, t_stride apart, scanned by one batched prefix sum
// whose workspace was sized for scan_batch rows; max_q = the longest query row of the views.
inline int gather_build(const GatherViews& both, int sides, int clouds, int64_t max_q, const GatherWorkspace& w,
                        int64_t t_rows, int64_t scan_n, int scan_batch, hipStream_t s) {
  const dim3 grid(iso_capped_grid(max_q, 256, 4096), clouds, sides);
  iso_zero_words(w.cnt, t_rows + 4, s);
  if (max_q > 0) hipLaunchKernelGGL(k_gather_pass<false>, grid, dim3(256), 0, s, both);
  const int rc = iso_prefix_sum(w.cnt, w.off, scan_n, sides * clouds, both.d[0].t_stride, w.scan_ws,
                                iso_prefix_sum_workspace_bytes(scan_n, scan_batch), (void*)s);
  if (rc != ISO_OK) return rc;
  if (max_q > 0) hipLaunchKernelGGL(k_gather_pass<true>, grid, dim3(256), 0, s, both);
  return ISO_OK;
}

}  // namespace
