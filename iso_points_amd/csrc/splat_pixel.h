// What one pixel of the splat raster does, shared by the tile raster (splat_raster.hip) and the reference's coarse / fine
// interface (splat_bins.hip) so that the compatibility paths cannot drift from the hot one: the inside test, the K-best
// list's epilogue (depth-merging cut, outputs, visible marks), the deep list for points_per_pixel > 32 and the fused
// compositing.  Reference: CheckPixelInsidePoint and the naive kernel's write-back, DSS/csrc/rasterize_points.cu:79-97,
// :182-211; compositing SurfaceSplattingRenderer.forward, DSS/core/renderer.py:53-78.
#pragma once
#include "splat_frame.h"
#include "kbest.h"

#pragma clang fp contract(off)

namespace {

// CheckPixelInsidePoint for the pixel at (dx, dy) from the point's centre: the box test (rasterize_points.cu:92), then
// q = a dx^2 + b dx dy + c dy^2 (:94) against the cutoff (:96).  q is written when the box test passes.  k_raster_deep
// and both fine kernels call it; k_raster's two sites are these lines written out (see there).
__device__ __forceinline__ bool pixel_inside_point(float dx, float dy, float a, float b, float c, float rx, float ry,
                                                   float cut, float& q) {
  if (fabsf(dx) > rx || fabsf(dy) > ry) return false;
  q = a * dx * dx + b * dx * dy + c * dy * dy;
  return !(q > cut);
}

// optional epilogue of the raster kernels: the compositing of k_composite for the pixel just finished
// (same arithmetic, same order; saves re-reading the K-deep lists)
struct CompositeArgs {
  const float* scaler;   // null: no compositing
  const float* feat;
  float* img;            // (N,S,S,C+1)
  int C, norm;
  float eps;
  uint8_t* vis;          // null, or (P,) flags: every point written to a pixel's list is marked 1 (k_mark_visible's pass)
};

// A list is anything with z[j], q[j], id[j] and live(j): a KBest in registers (KMAX > 0: the loop over its KMAX slots
// unrolls) or a DeepList in the pixel's output rows (KMAX == 0: K is the only bound).
template <int KMAX, class List>
__device__ __forceinline__ void composite_pixel(const List& best, int K, float z0, float depth_thres, bool hit,
                                                const CompositeArgs& ca, int64_t pix) {
  float sw = 0.f;
  float acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;
  // One loop for both kinds of list: KMAX slots, fully unrolled, or K rows, not unrolled.  (The plainer spellings --
  // the body in a lambda under `if constexpr`, or no pragma -- change the machine code of k_raster / k_raster_merge.)
  const int slots = KMAX > 0 ? KMAX : K;
#pragma unroll KMAX > 0 ? KMAX : 1
  for (int j = 0; j < slots; ++j) {
    if (j < K) {
      const bool ok = best.live(j) && !((best.z[j] - z0) > depth_thres);
      if (ok) {
        const int p = best.id[j];
        const float w = expf(-0.5f * best.q[j]) * ca.scaler[p];
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < ca.C) acc[c] += w * ca.feat[(int64_t)p * ca.C + c];
        sw += w;
      }
    }
  }
  float d = 1.0f;
  if (ca.norm) d = sw > ca.eps ? sw : ca.eps;
#pragma unroll
  for (int c = 0; c < 8; ++c) if (c < ca.C) ca.img[pix * (ca.C + 1) + c] = ca.norm ? acc[c] / d : acc[c];
  ca.img[pix * (ca.C + 1) + ca.C] = hit ? 1.0f : 0.0f;
}

// The end of a pixel whose K-best list is in registers: occupancy, the depth-merging cut (an entry further than
// depth_thres behind the front one is dropped) and the three list rows.  k_fine_bins calls it.  k_raster and
// k_raster_merge carry these statements themselves, with the visible marks and the image behind them: a call there
// reorders their stores' address arithmetic, and their machine code is pinned -- a change here is a change there.
template <int KMAX>
__device__ __forceinline__ void write_pixel_lists(const PixK<KMAX>& best, int K, float depth_thres, int64_t pix,
                                                  int32_t* __restrict__ idx_out, float* __restrict__ zbuf_out,
                                                  float* __restrict__ q_out, float* __restrict__ occ_out) {
  const float z0 = best.z[0];
  occ_out[pix] = z0 < FLT_MAX ? 1.0f : 0.0f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < K) {
      const bool ok = best.z[j] < FLT_MAX && !((best.z[j] - z0) > depth_thres);
      idx_out[pix * K + j] = ok ? best.id[j] : -1;
      zbuf_out[pix * K + j] = ok ? best.z[j] : -1.0f;
      q_out[pix * K + j] = ok ? best.q[j] : -1.0f;
    }
  }
}

// points_per_pixel above 32 (the reference allows 150, rasterization_utils.cuh:18): the K-best list of a pixel does not
// fit its thread's registers, so it lives where it ends up anyway -- in the pixel's rows of the output arrays -- and a
// hit is inserted by shifting the tail in global memory.  Same (z, id) order and the same cut as the register list;
// built for completeness, not for speed (a list this deep is a debugging setting).
struct DeepList {
  int32_t* id;                 // the pixel's rows of idx / zbuf / qvalue
  float* z;
  float* q;
  int K, have;
  float wz;                    // worst entry of a full list
  int wi;
  __device__ __forceinline__ DeepList(int32_t* idx_out, float* zbuf_out, float* q_out, int64_t pix, int K_)
      : id(idx_out + pix * K_), z(zbuf_out + pix * K_), q(q_out + pix * K_), K(K_), have(0), wz(FLT_MAX), wi(0x7fffffff) {}
  __device__ __forceinline__ bool live(int j) const { return j < have; }
  __device__ __forceinline__ void push(float pz, int p, float pq) {
    if (have == K && !(pz < wz || (pz == wz && p < wi))) return;
    int j = have < K ? have : K - 1;        // the slot that opens (the worst entry drops out of a full list)
    while (j > 0) {
      const float zj = z[j - 1];
      const int ij = id[j - 1];
      if (!(pz < zj || (pz == zj && p < ij))) break;
      z[j] = zj; id[j] = ij; q[j] = q[j - 1];
      --j;
    }
    z[j] = pz; id[j] = p; q[j] = pq;
    if (have < K) ++have;
    if (have == K) { wz = z[K - 1]; wi = id[K - 1]; }
  }
  __device__ __forceinline__ float front() const { return have > 0 ? z[0] : FLT_MAX; }
  // occupancy, visible marks (vis may be null) and the cut: dropped and unused slots become -1
  __device__ __forceinline__ void finish(float depth_thres, float* __restrict__ occ_out, int64_t pix, uint8_t* vis) {
    const float z0 = front();
    occ_out[pix] = have > 0 ? 1.0f : 0.0f;
    for (int j = 0; j < K; ++j) {
      const bool ok = j < have && !((z[j] - z0) > depth_thres);
      if (ok && vis) vis[id[j]] = 1;
      if (!ok) { id[j] = -1; z[j] = -1.0f; q[j] = -1.0f; }
    }
  }
};

}  // namespace
