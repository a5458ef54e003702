// The N-rank halo exchange of the brick grid (bricks.h): what a rank exports to and imports from the others between the
// header write (iso_bricks_params) and the build (iso_bricks_build; both in bricks.hip), which counts and scatters the
// imported records beside the rank's own.  The Python side is iso_points_amd/dist.py.
#include "bricks.h"

#pragma clang fp contract(off)

namespace {

// ---- halo exchange between x-slabs (one rank per GPU) ---------------------------------------------
// Every rank's LOCAL bounding box is known to all (ranges: (world, 8) floats, iso_points_bbox layout).
// Rank k's queries live in fine x-cells [fx(min_k), fx(max_k)]; their 3x3x3 neighbourhoods reach one
// fine cell further, so rank j exports exactly its points whose fine x-cell lies in that widened range
// of some other rank, and rank k imports, from what all ranks exported, those in its own widened range.
// Buffers: float4[2][cap + 1]; word 0 of record 0 is the record count (int bits).
__global__ __launch_bounds__(256) void k_halo_export(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                     const int32_t* __restrict__ payload, int64_t n_own,
                                                     const BrickHdr* __restrict__ hp, const float* __restrict__ ranges,
                                                     int world, int rank, int halo, float4* __restrict__ out, int cap) {
  const BrickHdr h = *hp;
  __shared__ int s_app[17];
  int32_t* counter = reinterpret_cast<int32_t*>(out);
  const int64_t span = (int64_t)gridDim.x * 1024;
  for (int64_t i0 = (int64_t)blockIdx.x * 1024; i0 < n_own; i0 += span) {
    bool take[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = i0 + q * 256 + threadIdx.x;
      take[q] = false;
      if (i < n_own) {
        const int fx = bk_fine(pts[i * 3], h.mn[0], h.inv_f, h.nf[0]);
        for (int k = 0; k < world; ++k) {
          if (k == rank) continue;
          const int lo = bk_fine(ranges[k * 8], h.mn[0], h.inv_f, h.nf[0]) - halo;
          const int hi = bk_fine(ranges[k * 8 + 4], h.mn[0], h.inv_f, h.nf[0]) + halo;
          take[q] = take[q] || (fx >= lo && fx <= hi);
        }
      }
    }
    int slot[4];
    iso_block_append4(take, counter, s_app, slot);      // (the count may pass cap: the importer clamps and reports it)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (slot[q] >= 0 && slot[q] < cap) {
        const int64_t i = i0 + q * 256 + threadIdx.x;
        out[1 + slot[q]] = make_float4(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], __int_as_float(h.id_base + (int)i));
        float4 u = make_float4(0.f, 0.f, 0.f, __int_as_float(payload ? payload[i] : 0));
        if (nrm) { u.x = nrm[i * 3]; u.y = nrm[i * 3 + 1]; u.z = nrm[i * 3 + 2]; }
        out[(int64_t)cap + 1 + 1 + slot[q]] = u;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_halo_import(const float4* __restrict__ gathered, int world, int rank, int cap,
                                                     int halo, BrickHdr* __restrict__ hp, const float* __restrict__ ranges,
                                                     float4* __restrict__ imp0, float4* __restrict__ imp1,
                                                     int32_t* __restrict__ imp_count, int imp_cap,
                                                     int32_t* __restrict__ counters) {
  const int src = blockIdx.y;
  const BrickHdr h = *hp;
  const int lo = bk_fine(ranges[rank * 8], h.mn[0], h.inv_f, h.nf[0]) - halo;
  const int hi = bk_fine(ranges[rank * 8 + 4], h.mn[0], h.inv_f, h.nf[0]) + halo;
  if (src == rank) {
    // everything the cloud holds in fine x-cells [lo, hi] is on this rank now: the tail kernels check their
    // search balls against this range (a query that needs more is counted, IsoCycle.check reports it)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      hp->x_lo = lo <= 0 ? -FLT_MAX : h.mn[0] + (float)lo * h.f;
      hp->x_hi = hi >= h.nf[0] - 1 ? FLT_MAX : h.mn[0] + (float)(hi + 1) * h.f;
      // the work list of the fused kernels (k_brick_offsets*) skips the bricks outside the rank's own columns: their
      // records are candidates only, and a workgroup that staged one found no query (half the list at N = 8)
      hp->own_bx_lo = (lo + halo) >> 2;
      hp->own_bx_hi = (hi - halo) >> 2;
    }
    return;
  }
  const float4* blk = gathered + (int64_t)src * 2 * (cap + 1);
  int cnt = __float_as_int(blk[0].x);
  if (cnt > cap) { cnt = cap; if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(&counters[4], 1); }   // the exporter overflowed
  __shared__ int s_app[17];
  const int span = gridDim.x * 1024;
  for (int j0 = blockIdx.x * 1024; j0 < cnt; j0 += span) {
    bool take[4];
    float4 p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + q * 256 + threadIdx.x;
      take[q] = false;
      p[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < cnt) {
        p[q] = blk[1 + j];
        const int fx = bk_fine(p[q].x, h.mn[0], h.inv_f, h.nf[0]);
        take[q] = fx >= lo && fx <= hi;
      }
    }
    int slot[4];
    iso_block_append4(take, imp_count, s_app, slot);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (slot[q] < 0) continue;
      if (slot[q] < imp_cap) { imp0[slot[q]] = p[q]; imp1[slot[q]] = blk[(int64_t)cap + 1 + 1 + j0 + q * 256 + threadIdx.x]; }
      else atomicAdd(&counters[5], 1);                                                                // import overflow
    }
  }
}

}  // namespace

// ================================================================================================
extern "C" int iso_halo_export(void* workspace, const float* points, const float* normals, const int32_t* payload,
                               int64_t n_own, const float* rank_boxes, int world, int rank, int halo_cells,
                               float* export_buf, int64_t capacity, void* stream) {
  ISO_REQUIRE(workspace && rank_boxes && export_buf && world >= 1 && rank >= 0 && rank < world && capacity >= 0 &&
                  capacity < (1ll << 30) && (points || n_own == 0),
              ISO_ERR_INVALID, "iso_halo_export: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  iso_zero_words(export_buf, 4, s);
  if (n_own > 0)
    hipLaunchKernelGGL(k_halo_export, dim3(iso_stream_grid(n_own, 1024)), dim3(256), 0, s, points, normals, payload, n_own,
                       (const BrickHdr*)workspace, rank_boxes, world, rank, halo_cells, (float4*)export_buf, (int)capacity);
  ISO_CHECK_LAUNCH("iso_halo_export");
  return ISO_OK;
}

extern "C" int iso_halo_import(void* workspace, int64_t n_max, const float* gathered, const float* rank_boxes, int world,
                               int rank, int halo_cells, int64_t capacity, float* import_rec0, float* import_rec1,
                               int32_t* import_count, int64_t import_capacity, void* stream) {
  ISO_REQUIRE(workspace && gathered && rank_boxes && import_rec0 && import_rec1 && import_count && world >= 1 &&
                  rank >= 0 && rank < world && capacity >= 0 && import_capacity >= 0 && halo_cells >= 1,
              ISO_ERR_INVALID, "iso_halo_import: bad arguments");
  const BrickWs w = bricks_carve(workspace, n_max);
  hipStream_t s = (hipStream_t)stream;
  iso_zero_words(import_count, 1, s);
  if (capacity > 0 && world > 1)
    hipLaunchKernelGGL(k_halo_import, dim3(iso_stream_grid(capacity, 256) > 64 ? 64 : iso_stream_grid(capacity, 256), world),
                       dim3(256), 0, s, (const float4*)gathered, world, rank, (int)capacity, halo_cells, w.hdr, rank_boxes,
                       (float4*)import_rec0, (float4*)import_rec1, import_count, (int)import_capacity, w.counters);
  ISO_CHECK_LAUNCH("iso_halo_import");
  return ISO_OK;
}
