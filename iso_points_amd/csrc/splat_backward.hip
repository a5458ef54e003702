// EWA surface splatting for gfx950, stage 5 of 6: the (deterministic) backward pass -- visible marks, the xy gradient
// of the occupancy image and the z gradient in 64-bit fixed point.
//
// Reference semantics
//   backward : EllipticalRasterizer.backward (rasterizer.py:841-968) +
//              RasterizePointsBackwardCudaFastKernel
//              (rasterize_points_backward.cu:85-178) + ZbufBackwardKernel
//              (rasterize_points.cu:823-846)
//
// Backward is point-major: every visible point walks the pixels of its
// support in image order and accumulates in registers -- no float atomics, so
// gradients are bit-stable (the reference's gpuAtomicAdd order is not).
#include <float.h>
#include "splat_frame.h"

#pragma clang fp contract(off)

// Riders (workgroups past the kernel's own grid, see iso_splat_backward): work of the z pass that depends on nothing the
// host kernel of the launch does, only on launches before it.
struct ZScale;
struct ZRider {                  // k_splat_backward's: max |grad_zbuf| (k_z_absmax's pass); k_splat_backward_heavy's: the
  const float* gz; int64_t n;    // conversion of the fixed-point sums (k_z_finish_clouds's pass)
  ZScale* zs; int blocks;        // blocks == 0: no riders
  const long long* acc; float* grad; int terms_log2;
};
__device__ void z_absmax_body(const float* __restrict__ gz, int64_t n, ZScale* __restrict__ zs, int block, int nblocks);
__device__ void z_finish_body(const long long* __restrict__ acc, const ZScale* __restrict__ zs, const int64_t* __restrict__ first,
                              const int64_t* __restrict__ num, int n_clouds, float* __restrict__ grad, int terms_log2,
                              int block, int nblocks);

namespace {

// ---------------------------------------------------------------- backward
// visible[p] = 1 for every point listed in a pixel whose first slot is filled
// (rasterizer.py:850-856)
__global__ void k_mark_visible(const int32_t* __restrict__ idx0, int K, int64_t npix,
                               uint8_t* __restrict__ visible, int64_t view_stride = 0) {
  const int32_t* __restrict__ idx = idx0 + (int64_t)blockIdx.y * view_stride * K;   // (N views of a band: grid.y)
  if ((K & 3) == 0 && ((uintptr_t)idx & 15) == 0) {                    // four list entries per 16-byte load
    const int4* __restrict__ idx4 = reinterpret_cast<const int4*>(idx);
    const int64_t nq = npix * (K / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
      const int4 p = idx4[i];
      if (p.x >= 0) visible[p.x] = 1;
      if (p.y >= 0) visible[p.y] = 1;
      if (p.z >= 0) visible[p.z] = 1;
      if (p.w >= 0) visible[p.w] = 1;
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (idx[i * K] < 0) continue;
    for (int k = 0; k < K; ++k) {
      const int p = idx[i * K + k];
      if (p >= 0) visible[p] = 1;
    }
  }
}

// ZbufBackwardKernel (rasterize_points.cu:823-846): z_grad[idx] += grad_zbuf, zeros skipped,
// stop at the first idx < 0.  Atomic scatter (order-dependent like the reference's).
__global__ void k_zbuf_scatter(const int32_t* __restrict__ idx, const float* __restrict__ gz,
                               int K, int64_t npix, float* __restrict__ z_grad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix;
       i += (int64_t)gridDim.x * blockDim.x) {
    for (int k = 0; k < K; ++k) {
      const float g = gz[i * K + k];
      if (g == 0.0f) continue;
      const int p = idx[i * K + k];
      if (p < 0) break;
      atomicAdd(&z_grad[p], g);
    }
  }
}

// coarse map of 8x8 pixel blocks that hold a non-zero occupancy gradient
constexpr int GB = 8;
struct BlkGeo { int NBx, NBy, NB2x, NB2y; };
static inline BlkGeo make_blk(int H, int W) {
  BlkGeo g;
  g.NBx = (W + GB - 1) / GB; g.NBy = (H + GB - 1) / GB; g.NB2x = (g.NBx + 7) / 8; g.NB2y = (g.NBy + 7) / 8;
  return g;
}

// Gradient maps of the occupancy image, three levels in one launch: one WAVE per 64x64-pixel super block, lane = one
// of its 8x8 blocks (lane % 8 = block column).  A lane reads the 8 rows of its block as 2 x 16 bytes each when the row
// is aligned and writes the block's pixel mask (bit 8 ry + rx: that pixel carries a gradient); the flags of a row of
// eight blocks are one byte (the ballot), the super block's flag says whether any of them is set.  Workgroup 0 also
// clears the few words the later passes count into (heavy-point list length, z scale): no clearing launches.
__global__ __launch_bounds__(256) void k_grad_maps(const float* __restrict__ grad_occ, Frame F, BlkGeo G, int N,
                                                   unsigned long long* __restrict__ pixmask /*(N, NBy, NBx)*/,
                                                   uint8_t* __restrict__ rowbytes /*(N, NBy, NB2x)*/,
                                                   uint8_t* __restrict__ blk2 /*(N, NB2y, NB2x)*/,
                                                   int32_t* __restrict__ clear_a, int n_clear_a,
                                                   int32_t* __restrict__ clear_b, int n_clear_b) {
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < n_clear_a) clear_a[threadIdx.x] = 0;
    if (clear_b && (int)threadIdx.x < n_clear_b) clear_b[threadIdx.x] = 0;
  }
  const int lane = threadIdx.x & 63;
  const int64_t total = (int64_t)N * G.NB2x * G.NB2y;
  for (int64_t sb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); sb < total; sb += (int64_t)gridDim.x * 4) {
    const int sx = sb % G.NB2x, sy = (sb / G.NB2x) % G.NB2y, n = sb / ((int64_t)G.NB2x * G.NB2y);
    const int bx = sx * 8 + (lane & 7), by = sy * 8 + (lane >> 3);
    unsigned long long m = 0ull;
    if (bx < G.NBx && by < G.NBy) {
      const int x0 = bx * GB, x1 = min(F.W, x0 + GB);
      for (int y = by * GB; y < min(F.H, (by + 1) * GB); ++y) {
        const float* row = grad_occ + ((int64_t)n * F.H + y) * F.W;
        unsigned bits = 0u;
        if (x1 - x0 == GB && (((uintptr_t)(row + x0)) & 15) == 0) {
          const float4 a = *reinterpret_cast<const float4*>(row + x0), c = *reinterpret_cast<const float4*>(row + x0 + 4);
          bits = (unsigned)(a.x != 0.f) | ((unsigned)(a.y != 0.f) << 1) | ((unsigned)(a.z != 0.f) << 2) | ((unsigned)(a.w != 0.f) << 3) |
                 ((unsigned)(c.x != 0.f) << 4) | ((unsigned)(c.y != 0.f) << 5) | ((unsigned)(c.z != 0.f) << 6) | ((unsigned)(c.w != 0.f) << 7);
        } else {
          for (int x = x0; x < x1; ++x) bits |= (unsigned)(row[x] != 0.0f) << (x - x0);
        }
        m |= (unsigned long long)bits << (8 * (y - by * GB));
      }
      pixmask[((int64_t)n * G.NBy + by) * G.NBx + bx] = m;
    }
    const unsigned long long bal = __ballot(m != 0ull);
    if ((lane & 7) == 0 && by < G.NBy) rowbytes[((int64_t)n * G.NBy + by) * G.NB2x + sx] = (uint8_t)((bal >> (8 * (lane >> 3))) & 0xffull);
    if (lane == 0) blk2[sb] = bal ? 1 : 0;
  }
}

// output-pixel range [lo,hi] (after the axis flip) whose centres may lie within c +- r
__device__ __forceinline__ bool out_range(float c, float r, int n, float e, int m, int& lo, int& hi) {
  int a, b;
  if (!pixel_range(c, r, n, e, m, a, b)) return false;
  lo = n - 1 - b;
  hi = n - 1 - a;
  return true;
}

// xy contribution of one pixel to one point (shared by both backward kernels)
__device__ __forceinline__ void occ_term(float g, float dx, float dy, float rx, float ry, float sx,
                                         float sy, float r2, int rect_mode, float radii_s, float& gx,
                                         float& gy) {
  if (g == 0.0f) return;
  const float dist2 = dx * dx + dy * dy;
  bool outside;
  if (rect_mode) {  // rasterize_points.cu:726-746 (slow CUDA kernel)
    if (fabsf(dx) > sx || fabsf(dy) > sy) return;
    outside = (fabsf(dx) > sx / radii_s) || (fabsf(dy) > sy / radii_s);
  } else {          // rasterize_points_backward.cu:156-161 (fast kernel)
    if (dist2 > r2) return;
    outside = (fabsf(dx) > rx) || (fabsf(dy) > ry);
  }
  if (g > 0.0f && outside) return;
  const float denom = iso_eps_denom(dist2, 1e-10f);
  gx += dx / denom * g;
  gy += dy / denom * g;
}

// Pass 1, one lane per point, the cheap part of the xy gradient: a point whose support touches no 64x64
// super block with a gradient is done (xy = 0); the others are appended to the heavy list.
__global__ __launch_bounds__(256) void k_splat_backward(
    const float* __restrict__ pts, const float* __restrict__ radii,
    const uint8_t* __restrict__ visible, const float* __restrict__ rs,
    const int64_t* __restrict__ first, const int64_t* __restrict__ num,
    const uint8_t* __restrict__ blk2, BlkGeo G, Frame F, int rect_mode, float radii_s,
    int32_t* __restrict__ heavy, int32_t* __restrict__ heavy_count, float* __restrict__ grad,
    long long* __restrict__ zacc /* fixed-point z accumulators, cleared here row by row (NULL: none) */,
    ZRider rider, int own_blocks) {
  if ((int)blockIdx.x >= own_blocks) {                 // riders: blockIdx.y == 0 only
    if (blockIdx.y == 0) z_absmax_body(rider.gz, rider.n, rider.zs, blockIdx.x - own_blocks, rider.blocks);
    return;
  }
  const int n = blockIdx.y;
  const int64_t len = num[n], base = first[n];
  const float r = rect_mode ? 0.f : rs[n];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // 1024 points per round and workgroup: the heavy list is appended to with ONE returning atomic per round
  // (one per 256 points made ~8 k same-address atomics the critical path of the kernel)
  __shared__ int s_wcnt[4][4], s_base;
  const int64_t span = (int64_t)own_blocks * 1024;
  for (int64_t i0 = (int64_t)blockIdx.x * 1024; i0 < len; i0 += span) {
    bool is_heavy[4];
    int64_t pp[4];
    unsigned long long bal[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = i0 + k * 256 + threadIdx.x;
      is_heavy[k] = false;
      pp[k] = -1;
      if (i < len) {
        const int64_t p = base + i;
        pp[k] = p;
        const float px = pts[p * 3], py = pts[p * 3 + 1], pz = pts[p * 3 + 2];
        const float rx = radii[p * 2], ry = radii[p * 2 + 1];
        const bool vis = (!visible || visible[p]);
        grad[p * 3] = 0.f; grad[p * 3 + 1] = 0.f; grad[p * 3 + 2] = 0.f;   // z: k_z_scatter / k_z_finish
        if (zacc) zacc[p] = 0;
        const float sx = rect_mode ? rx * radii_s : r, sy = rect_mode ? ry * radii_s : r;
        // (the fast kernel skips points outside the image: rasterize_points_backward.cu:101-103; here: outside the frame)
        if (vis && !(pz < 0.f || fabsf(py) > F.ey || fabsf(px) > F.ex) && sx > 0.f && sy > 0.f) {
          int x0, x1, y0, y1;
          if (out_range(px, sx, F.W, F.ex, F.m, x0, x1) && out_range(py, sy, F.H, F.ey, F.m, y0, y1)) {
            for (int sy2 = y0 / 64; sy2 <= y1 / 64 && !is_heavy[k]; ++sy2)
              for (int sx2 = x0 / 64; sx2 <= x1 / 64; ++sx2)
                if (blk2[((int64_t)n * G.NB2y + sy2) * G.NB2x + sx2]) { is_heavy[k] = true; break; }
          }
        }
      }
      bal[k] = __ballot(is_heavy[k]);
      if (lane == 0) s_wcnt[k][wv] = __popcll(bal[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) tot += s_wcnt[q >> 2][q & 3];
      s_base = tot ? atomicAdd(heavy_count, tot) : 0;
    }
    __syncthreads();
    int b0 = s_base;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q == wv && is_heavy[k]) heavy[b0 + __popcll(bal[k] & ((1ull << lane) - 1ull))] = (int32_t)pp[k];
        b0 += s_wcnt[k][q];
      }
    }
    __syncthreads();
  }
}

// Pass 2, eight LANES per heavy point.  Measured on the cfg-3a cycle (tools/diag/heavy_count.py): 154 k heavy points whose
// discs (29.5 px radius: up to 81 blocks) hold 3.7 flagged blocks and 18 pixels with a gradient each -- the first form
// spent a wave per point (one pixel per lane, a block per round, a butterfly at the end): ~350 wave instructions for 18
// useful terms, the kernel was bound by exactly that (54 M VALU instructions per launch = 100 % of the issue rate).
// Here the eight lanes of a point read the row bytes of its disc (k_grad_maps; 4 block rows x 32 blocks per round, the
// words requested together) and walk its flagged blocks together; of a block's pixels that carry a gradient (pixel
// masks) lane j takes those on the diagonals (rx + ry) % 8 = j -- a silhouette arc crosses a block along a row, a column
// or the other diagonal, and dealing out block rows (or blocks) left such an arc to one or two lanes: 100 -> 43 us on
// the sparse gradient image of cfg 3a but 159 -> 228 us on the denser one of the SIREN cycle.  A lane adds its terms in
// image order, the eight partial sums meet in a fixed tree -> bit-stable, no atomics, independent of the launch geometry.
// (one lane per point: 100 -> 64 us, bound by the lane's chain of dependent loads at 2.4 waves per SIMD)
__global__ __launch_bounds__(256) void k_splat_backward_heavy(
    const float* __restrict__ pts, const float* __restrict__ radii, const float* __restrict__ rs,
    const int64_t* __restrict__ first, const int64_t* __restrict__ num, int n_clouds,
    const float* __restrict__ grad_occ, const unsigned long long* __restrict__ pixmask,
    const uint8_t* __restrict__ rowbytes, BlkGeo G, Frame F,
    int rect_mode, float radii_s, const int32_t* __restrict__ heavy,
    const int32_t* __restrict__ heavy_count, float* __restrict__ grad, ZRider rider, int own_blocks) {
  if ((int)blockIdx.x >= own_blocks) {
    z_finish_body(rider.acc, rider.zs, first, num, n_clouds, rider.grad, rider.terms_log2, blockIdx.x - own_blocks, rider.blocks);
    return;
  }
  const int count = *heavy_count;
  constexpr int LP = 8;                                   // lanes per point
  const int j = threadIdx.x & (LP - 1);
  unsigned long long diag = 0ull;                         // the pixels of an 8x8 block this lane takes: (rx + ry) % 8 = j
  for (int ry = 0; ry < 8; ++ry) diag |= 1ull << (8 * ry + ((j - ry) & 7));
  // (count rounded up: the lanes of a group leave the loop together, the shuffles below need all of them)
  for (int w = (blockIdx.x * blockDim.x + threadIdx.x) / LP; w < (count + 63) / 64 * 64; w += own_blocks * blockDim.x / LP) {
    const bool live = w < count;
    const int64_t p = live ? heavy[w] : 0;
    int n = 0;
    for (int c = 1; c < n_clouds; ++c) if (p >= first[c]) n = c;     // clouds are packed in order
    const float r = rect_mode ? 0.f : rs[n], r2 = r * r;
    const float px = pts[p * 3], py = pts[p * 3 + 1];
    const float rx = radii[p * 2], ry = radii[p * 2 + 1];
    const float sx = rect_mode ? rx * radii_s : r, sy = rect_mode ? ry * radii_s : r;
    int x0, x1, y0, y1;
    float gx = 0.f, gy = 0.f;
    if (live && out_range(px, sx, F.W, F.ex, F.m, x0, x1) && out_range(py, sy, F.H, F.ey, F.m, y0, y1)) {
      const float* __restrict__ gimg = grad_occ + (int64_t)n * F.H * F.W;
      const int bx0 = x0 / GB, bx1 = x1 / GB, by0 = y0 / GB, by1 = y1 / GB;
      // block rows per round: their flag words are requested together (1 / 2 / 4 / 8 / 16: 56 / 53 / 54 / 59 / 66 us on cfg 3a)
      constexpr int RY = 4;
      for (int cx = bx0 >> 3; cx <= bx1 >> 3; cx += 4) {  // 32 blocks (four row bytes = one unaligned word) per round
        // blocks of the window in this word, and of those the ones on this lane's diagonals
        const int ka = max(bx0 - cx * 8, 0), kb = min(bx1 - cx * 8, 31);
        const unsigned colwin = (0xffffffffu >> (31 - kb)) & (0xffffffffu << ka);
        for (int byc = by0; byc <= by1; byc += RY) {
          unsigned fl[RY];
#pragma unroll
          for (int t = 0; t < RY; ++t) {
            fl[t] = 0u;
            if (byc + t <= by1) {
              const uint8_t* rp = rowbytes + ((int64_t)n * G.NBy + byc + t) * G.NB2x + cx;
              unsigned wv;
              __builtin_memcpy(&wv, rp, 4);               // (bytes past the row's end belong to blocks outside the window)
              fl[t] = wv & colwin;
            }
          }
#pragma unroll
          for (int t = 0; t < RY; ++t) {
            const int by = byc + t;
            unsigned flags = fl[t];
            if (!flags) continue;
            // rows of the block inside the window, as a mask of whole bytes
            const int ra = max(y0 - by * GB, 0), rb = min(y1 - by * GB, GB - 1);
            const unsigned long long rowsel = (rb == 7 ? ~0ull : ((1ull << (8 * (rb + 1))) - 1ull)) & ~((1ull << (8 * ra)) - 1ull);
            while (flags) {
              const int k = __ffs((int)flags) - 1;
              flags &= flags - 1;
              const int bx = cx * 8 + k;
              // columns of the block inside the window, the same byte in every row
              const int ca = max(x0 - bx * GB, 0), cb = min(x1 - bx * GB, GB - 1);
              const unsigned long long colsel = (unsigned long long)((0xffu >> (7 - cb)) & (0xffu << ca)) * 0x0101010101010101ull;
              const unsigned long long win = rowsel & colsel;
              unsigned long long m = pixmask[((int64_t)n * G.NBy + by) * G.NBx + bx] & win;
              if (m == win && bx * GB + GB <= F.W && (F.W & 3) == 0 && (((uintptr_t)gimg) & 15) == 0) {
                // every pixel of the window's part of this block carries a gradient (a dense gradient image): lane j
                // takes pixel row j as two 16-byte loads, no bit scans
                if (j >= ra && j <= rb) {
                  const int yo = by * GB + j;
                  const float4* rowp = reinterpret_cast<const float4*>(gimg + (int64_t)yo * F.W + bx * GB);
                  const float4 ga = rowp[0], gb = rowp[1];
                  const float gv[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
                  const float dy = ndc_y(F.H - 1 - yo, F) - py;
#pragma unroll
                  for (int rxx = 0; rxx < GB; ++rxx)
                    if (rxx >= ca && rxx <= cb)
                      occ_term(gv[rxx], ndc_x(F.W - 1 - (bx * GB + rxx), F) - px, dy, rx, ry, sx, sy, r2, rect_mode, radii_s, gx, gy);
                }
                continue;
              }
              m &= diag;
              while (m) {
                const int b = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int yo = by * GB + (b >> 3), xo = bx * GB + (b & 7);
                const float g = gimg[(int64_t)yo * F.W + xo];
                occ_term(g, ndc_x(F.W - 1 - xo, F) - px, ndc_y(F.H - 1 - yo, F) - py, rx, ry, sx, sy, r2, rect_mode, radii_s, gx, gy);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = 1; o < LP; o <<= 1) {                    // fixed tree over the LP partial sums
      gx += __shfl_xor(gx, o);
      gy += __shfl_xor(gy, o);
    }
    if (live && j == 0) { grad[p * 3] = gx; grad[p * 3 + 1] = gy; }
  }
}

}  // namespace

// ===========================================================================
extern "C" int iso_splat_mark_visible(const int32_t* idx, int64_t n_pixels, int points_per_pixel,
                                      uint8_t* visible, void* stream) {
  ISO_REQUIRE(n_pixels >= 0 && points_per_pixel >= 1, ISO_ERR_INVALID, "iso_splat_mark_visible: bad sizes");
  if (n_pixels == 0) return ISO_OK;
  ISO_REQUIRE(idx && visible, ISO_ERR_INVALID, "iso_splat_mark_visible: null pointer");
  hipLaunchKernelGGL(k_mark_visible, dim3(iso_stream_grid(n_pixels, 256)), dim3(256), 0,
                     (hipStream_t)stream, idx, points_per_pixel, n_pixels, visible);
  ISO_CHECK_LAUNCH("iso_splat_mark_visible");
  return ISO_OK;
}

extern "C" int iso_splat_zbuf_backward(const int32_t* idx, const float* grad_zbuf,
                                       int64_t n_pixels, int points_per_pixel, float* z_grad,
                                       void* stream) {
  ISO_REQUIRE(n_pixels >= 0 && points_per_pixel >= 1, ISO_ERR_INVALID, "iso_splat_zbuf_backward: bad sizes");
  if (n_pixels == 0) return ISO_OK;
  ISO_REQUIRE(idx && grad_zbuf && z_grad, ISO_ERR_INVALID, "iso_splat_zbuf_backward: null pointer");
  hipLaunchKernelGGL(k_zbuf_scatter, dim3(iso_stream_grid(n_pixels, 256)), dim3(256), 0,
                     (hipStream_t)stream, idx, grad_zbuf, points_per_pixel, n_pixels, z_grad);
  ISO_CHECK_LAUNCH("iso_splat_zbuf_backward");
  return ISO_OK;
}

// ---- z gradient by pixel-major scatter in 64-bit fixed point -------------------------------------
// z_grad[p] = sum of grad_zbuf over the slots that list p (ZbufBackwardKernel, rasterize_points.cu:
// 823-846: zeros skipped, a row ends at the first idx < 0).  The reference scatters with float
// atomics (order-dependent).  Here every contribution is converted exactly to a 64-bit integer
// multiple of q = 2^-e (e chosen from max|grad| so that 2^44 * q >= max|grad|), added with integer
// atomics -- associative, so the result does not depend on the order -- and converted back once:
// the exactly rounded sum (error <= 2^-44 max|grad| per term), bit-stable from run to run.
struct ZScale { unsigned max_bits; int exp2; };

// |x| as ordered bits; a NaN or an Inf counts as 0: it poisons the points that receive it (z_scatter_one) and must not
// set the scale of all the others (on top of the maximum it leaves the exponent 0: every other sum rounds to an integer)
__device__ __forceinline__ unsigned z_mag(unsigned bits) {
  bits &= 0x7fffffffu;
  return bits < 0x7f800000u ? bits : 0u;
}

__device__ void z_absmax_body(const float* __restrict__ gz, int64_t n, ZScale* __restrict__ zs, int block, int nblocks) {
  __shared__ unsigned sm[4];
  unsigned m = 0u;
  const int64_t n4 = n / 4;
  const uint4* g4 = reinterpret_cast<const uint4*>(gz);
  const int64_t stride = (int64_t)nblocks * blockDim.x;
  int64_t i = (int64_t)block * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {                    // four requests in flight
    const uint4 v0 = g4[i], v1 = g4[i + stride], v2 = g4[i + 2 * stride], v3 = g4[i + 3 * stride];
    const unsigned a = max(max(z_mag(v0.x), z_mag(v0.y)), max(z_mag(v0.z), z_mag(v0.w)));
    const unsigned b = max(max(z_mag(v1.x), z_mag(v1.y)), max(z_mag(v1.z), z_mag(v1.w)));
    const unsigned c = max(max(z_mag(v2.x), z_mag(v2.y)), max(z_mag(v2.z), z_mag(v2.w)));
    const unsigned d = max(max(z_mag(v3.x), z_mag(v3.y)), max(z_mag(v3.z), z_mag(v3.w)));
    m = max(m, max(max(a, b), max(c, d)));
  }
  for (; i < n4; i += stride) {
    const uint4 v = g4[i];
    const unsigned a = max(z_mag(v.x), z_mag(v.y)), b = max(z_mag(v.z), z_mag(v.w));
    m = max(m, max(a, b));
  }
  for (int64_t t = n4 * 4 + (int64_t)block * blockDim.x + threadIdx.x; t < n; t += stride)
    m = max(m, z_mag(__float_as_uint(gz[t])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    if (m) atomicMax(&zs->max_bits, m);
  }
}

__global__ __launch_bounds__(256) void k_z_absmax(const float* __restrict__ gz0, int64_t n, ZScale* __restrict__ zs,
                                                  int64_t view_stride = 0) {
  z_absmax_body(gz0 + (int64_t)blockIdx.y * view_stride, n, zs, blockIdx.x, gridDim.x);
}

// terms_log2 = ceil(log2(max number of slots that can list one point)) = ceil(log2(S*S)): every term is
// < 2^(61 - terms_log2) in magnitude after scaling, so no sum of them reaches 2^61 -- the range kept for
// the NaN / Inf poison (a point that received one stays at >= 2^61 whatever else is added).
__device__ __forceinline__ int z_exponent(unsigned max_bits, int terms_log2) {
  int e = 0;
  if (max_bits != 0u && max_bits < 0x7f800000u) {
    int ex;
    (void)frexpf(__uint_as_float(max_bits), &ex);      // max = f * 2^ex, f in [0.5,1)
    e = 61 - terms_log2 - ex;
  }
  return e;
}
__global__ void k_z_scale(ZScale* zs, int terms_log2) { zs->exp2 = z_exponent(zs->max_bits, terms_log2); }

__device__ __forceinline__ void z_scatter_one(int p, float g, int e, long long* __restrict__ acc) {
  if (g == 0.0f) return;
  if (g != g || fabsf(g) > 3.0e38f) {                                // poison: the point ends up NaN
    atomicMax(&acc[p], 1ll << 62);
    return;
  }
  const long long q = __double2ll_rn(ldexp((double)g, e));
  atomicAdd(reinterpret_cast<unsigned long long*>(&acc[p]), (unsigned long long)q);
}

// terms_log2 >= 0: the exponent is derived here from zs->max_bits (no k_z_scale launch in between); < 0: zs->exp2
__global__ void k_z_scatter(const int32_t* __restrict__ idx0, const float* __restrict__ gz0, int K, int64_t npix,
                            const ZScale* __restrict__ zs, long long* __restrict__ acc, int64_t view_stride = 0,
                            int terms_log2 = -1) {
  const int32_t* __restrict__ idx = idx0 + (int64_t)blockIdx.y * view_stride * K;
  const float* __restrict__ gz = gz0 + (int64_t)blockIdx.y * view_stride * K;
  const int e = terms_log2 >= 0 ? z_exponent(zs->max_bits, terms_log2) : zs->exp2;
  if ((K & 3) == 0 && (((uintptr_t)idx | (uintptr_t)gz) & 15) == 0) {   // a pixel's lists as 16-byte loads
    const int4* __restrict__ idx4 = reinterpret_cast<const int4*>(idx);
    const float4* __restrict__ gz4 = reinterpret_cast<const float4*>(gz);
    const int64_t nq = npix * (K / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
      // the gradient first: four slots without one (a loss on the front-most depth: every second quad) need no index read,
      // and the two loads of a quad that has one are independent
      const float4 g = gz4[i];
      if (g.x == 0.0f && g.y == 0.0f && g.z == 0.0f && g.w == 0.0f) continue;
      const int4 p = idx4[i];
      if (p.x < 0) continue;                                         // -1 padding is a suffix of a pixel's list
      z_scatter_one(p.x, g.x, e, acc);
      if (p.y >= 0) z_scatter_one(p.y, g.y, e, acc);
      if (p.z >= 0) z_scatter_one(p.z, g.z, e, acc);
      if (p.w >= 0) z_scatter_one(p.w, g.w, e, acc);
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    for (int k = 0; k < K; ++k) {
      const int p = idx[i * K + k];
      if (p < 0) break;
      z_scatter_one(p, gz[i * K + k], e, acc);
    }
  }
}

__global__ void k_z_finish(const long long* __restrict__ acc, const ZScale* __restrict__ zs, int64_t n,
                           float* __restrict__ grad, int terms_log2 = -1) {
  const int e = terms_log2 >= 0 ? z_exponent(zs->max_bits, terms_log2) : zs->exp2;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const long long a = acc[p];
    float z = (float)ldexp((double)a, -e);
    if (a >= (1ll << 61) || a <= -(1ll << 61)) z = __builtin_nanf("");
    grad[p * 3 + 2] = z;
  }
}

// the same over the rows of the clouds only (grid.y = cloud): rows of the packed arrays that belong to no cloud keep
// what the caller put there, as in the xy pass
__device__ void z_finish_body(const long long* __restrict__ acc, const ZScale* __restrict__ zs, const int64_t* __restrict__ first,
                              const int64_t* __restrict__ num, int n_clouds, float* __restrict__ grad, int terms_log2,
                              int block, int nblocks) {
  const int e = z_exponent(zs->max_bits, terms_log2);
  for (int c = 0; c < n_clouds; ++c) {
    const int64_t len = num[c], base = first[c];
    for (int64_t i = (int64_t)block * blockDim.x + threadIdx.x; i < len; i += (int64_t)nblocks * blockDim.x) {
      const int64_t p = base + i;
      const long long a = acc[p];
      float z = (float)ldexp((double)a, -e);
      if (a >= (1ll << 61) || a <= -(1ll << 61)) z = __builtin_nanf("");
      grad[p * 3 + 2] = z;
    }
  }
}

__global__ void k_z_finish_clouds(const long long* __restrict__ acc, const ZScale* __restrict__ zs,
                                  const int64_t* __restrict__ first, const int64_t* __restrict__ num,
                                  float* __restrict__ grad, int terms_log2) {
  z_finish_body(acc, zs, first + blockIdx.y, num + blockIdx.y, 1, grad, terms_log2, blockIdx.x, gridDim.x);
}

static int64_t bwd_maps_bytes(int n_clouds, int image_size, int image_width) {
  const BlkGeo G = make_blk(image_size, image_width > 0 ? image_width : image_size);
  // pixel masks (8 B per 8x8 block), row bytes (one per eight blocks of a block row), super-block flags
  return (((int64_t)n_clouds * ((int64_t)G.NBx * G.NBy * 8 + (int64_t)G.NB2x * G.NBy + (int64_t)G.NB2x * G.NB2y)) + 63) / 64 * 64;
}
extern "C" int64_t iso_splat_backward_workspace_bytes(int n_clouds, int image_size, int image_width,
                                                      int64_t total_points) {
  if (total_points < 0) total_points = 0;
  // [block maps][heavy count (64 B) + heavy list (4 B/pt)][pad 16][ZScale 16 B][z accumulators 8 B/pt]
  return bwd_maps_bytes(n_clouds, image_size, image_width) + 64 + (4 * total_points + 15) / 16 * 16 + 16 + 8 * total_points;
}

extern "C" int iso_splat_backward(const float* points, const float* radii, const uint8_t* visible,
                                  const float* search_radius, const int64_t* first_idx,
                                  const int64_t* num_pts, int n_clouds, int64_t max_pts,
                                  const float* grad_occ, const int32_t* idx,
                                  const float* grad_zbuf, int image_size, int image_width, int points_per_pixel,
                                  int rect_mode, float radii_s, int64_t total_points,
                                  void* workspace, int64_t workspace_bytes, float* grad_points,
                                  void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && max_pts >= 0 && image_size > 0, ISO_ERR_INVALID, "iso_splat_backward: bad sizes");
  if (n_clouds == 0 || max_pts == 0) return ISO_OK;
  ISO_REQUIRE(points && radii && (search_radius || rect_mode) && first_idx && num_pts && grad_occ &&
                  grad_points && workspace && (!grad_zbuf || idx),
              ISO_ERR_INVALID, "iso_splat_backward: null pointer");
  ISO_REQUIRE(workspace_bytes >= iso_splat_backward_workspace_bytes(n_clouds, image_size, image_width, total_points),
              ISO_ERR_WORKSPACE, "iso_splat_backward: workspace too small");
  const Frame F = make_frame(image_size, image_width > 0 ? image_width : image_size);
  const BlkGeo G = make_blk(F.H, F.W);
  ISO_REQUIRE(F.H <= 2048 && F.W <= 2048, ISO_ERR_UNSUPPORTED, "iso_splat_backward: image sides must be <= 2048");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* pixmask = (unsigned long long*)workspace;            // (caller buffers are 16-byte aligned)
  uint8_t* rowbytes = (uint8_t*)(pixmask + (int64_t)n_clouds * G.NBx * G.NBy);
  uint8_t* blk2 = rowbytes + (int64_t)n_clouds * G.NB2x * G.NBy;
  int32_t* heavy_count = (int32_t*)((uint8_t*)workspace + bwd_maps_bytes(n_clouds, image_size, image_width));
  int32_t* heavy = heavy_count + 16;
  const bool with_z = grad_zbuf && total_points > 0;
  ZScale* zs = reinterpret_cast<ZScale*>((char*)(heavy_count) + 64 + (4 * total_points + 15) / 16 * 16);
  long long* zacc = reinterpret_cast<long long*>((char*)zs + 16);
  // block maps of the image gradient (both levels, one launch); it also clears the heavy-list length and the z scale
  {
    int gmaps = iso_div_up((int64_t)n_clouds * G.NB2x * G.NB2y, 4);
    hipLaunchKernelGGL(k_grad_maps, dim3(gmaps < 1 ? 1 : gmaps), dim3(256), 0, s, grad_occ, F, G, n_clouds, pixmask, rowbytes, blk2,
                       heavy_count, 16, with_z ? reinterpret_cast<int32_t*>(zs) : nullptr, 4);
  }
  int gx = iso_div_up(max_pts, 1024); if (gx > 8192) gx = 8192;
  // The z part (pixel-major, fixed point) is three passes -- max |grad_zbuf|, scatter, conversion -- of which only the
  // scatter is a launch of its own: the maximum rides in the xy launch below (it reads nothing that launch writes; the
  // scale was cleared by k_grad_maps), the conversion in the heavy-point launch at the end (which writes x and y only).
  const int64_t npix = (int64_t)n_clouds * F.H * F.W;
  int terms_log2 = 0;
  while ((1ll << terms_log2) < (int64_t)F.H * F.W) ++terms_log2;
  ZRider r1{nullptr, 0, zs, 0, nullptr, nullptr, 0}, r2 = r1;
  if (with_z) {
    int gm = iso_div_up(npix * points_per_pixel, 256 * 16); if (gm > 1024) gm = 1024; if (gm < 1) gm = 1;
    r1 = ZRider{grad_zbuf, npix * points_per_pixel, zs, gm, nullptr, nullptr, 0};
    r2 = ZRider{nullptr, 0, zs, iso_stream_grid(total_points, 256), zacc, grad_points, terms_log2};
  }
  // xy part point-major (z written as 0, the z accumulators of the rows cleared)
  hipLaunchKernelGGL(k_splat_backward, dim3(gx + r1.blocks, n_clouds), dim3(256), 0, s, points, radii, visible,
                     search_radius, first_idx, num_pts, blk2, G, F, rect_mode, radii_s, heavy,
                     heavy_count, grad_points, with_z ? zacc : nullptr, r1, gx);
  if (with_z)      // the exponent is derived from the maximum inside the kernels that need it (no scale launch in between)
    hipLaunchKernelGGL(k_z_scatter, dim3(iso_stream_grid(npix, 256)), dim3(256), 0, s, idx, grad_zbuf,
                       points_per_pixel, npix, zs, zacc, (int64_t)0, terms_log2);
  // eight lanes per heavy point; the cost of a point varies with the gradient pixels under its disc, so the list is spread
  // over short-lived workgroups (a workgroup past the end of the list reads the count and leaves)
  constexpr int heavy_grid = 4096;
  hipLaunchKernelGGL(k_splat_backward_heavy, dim3(heavy_grid + r2.blocks), dim3(256), 0, s, points, radii, search_radius,
                     first_idx, num_pts, n_clouds, grad_occ, pixmask, rowbytes, G, F, rect_mode, radii_s,
                     heavy, heavy_count, grad_points, r2, heavy_grid);
  ISO_CHECK_LAUNCH("iso_splat_backward");
  return ISO_OK;
}

// ---- the z gradient in pieces (N ranks: every rank scatters the pixels of its own tile rows; the
// 64-bit accumulators are summed over the ranks before the finish; the scale comes from the global
// max |grad|).  zscale: 2 ints [max |grad| bits, exponent].
extern "C" int iso_splat_z_absmax(const float* grad_zbuf, int64_t n, int32_t* zscale, void* stream) {
  ISO_REQUIRE(zscale && n >= 0 && (grad_zbuf || n == 0), ISO_ERR_INVALID, "iso_splat_z_absmax: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  iso_zero_words(zscale, 2, s);
  if (n > 0) {
    int gm = iso_div_up(n, 256 * 16); if (gm > 1024) gm = 1024; if (gm < 1) gm = 1;
    hipLaunchKernelGGL(k_z_absmax, dim3(gm), dim3(256), 0, s, grad_zbuf, n, reinterpret_cast<ZScale*>(zscale));
  }
  ISO_CHECK_LAUNCH("iso_splat_z_absmax");
  return ISO_OK;
}

extern "C" int iso_splat_z_scatter(const int32_t* idx, const float* grad_zbuf, int64_t n_pixels, int points_per_pixel,
                                   int64_t pixels_per_view, int32_t* zscale, int64_t* acc, void* stream) {
  ISO_REQUIRE(zscale && acc && n_pixels >= 0 && points_per_pixel >= 1 && pixels_per_view > 0 && ((idx && grad_zbuf) || n_pixels == 0),
              ISO_ERR_INVALID, "iso_splat_z_scatter: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int terms_log2 = 0;
  while ((1ll << terms_log2) < pixels_per_view) ++terms_log2;
  hipLaunchKernelGGL(k_z_scale, dim3(1), dim3(1), 0, s, reinterpret_cast<ZScale*>(zscale), terms_log2);
  if (n_pixels > 0)
    hipLaunchKernelGGL(k_z_scatter, dim3(iso_stream_grid(n_pixels, 256)), dim3(256), 0, s, idx, grad_zbuf, points_per_pixel,
                       n_pixels, reinterpret_cast<const ZScale*>(zscale), reinterpret_cast<long long*>(acc));
  ISO_CHECK_LAUNCH("iso_splat_z_scatter");
  return ISO_OK;
}

// The three band calls of a cycle for all views at once (grid.y = view): the same kernels on
// idx / grad_zbuf + v * view_pixels * K for v < n_views (the band's rows of every view of an (N,H,W,K) array).
extern "C" int iso_splat_band_marks(const int32_t* idx, const float* grad_zbuf, int n_views, int64_t view_pixels,
                                    int64_t band_pixels, int points_per_pixel, uint8_t* visible, int32_t* zscale,
                                    void* stream) {
  ISO_REQUIRE(zscale && n_views >= 0 && view_pixels >= band_pixels && band_pixels >= 0 && points_per_pixel >= 1,
              ISO_ERR_INVALID, "iso_splat_band_marks: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  iso_zero_words(zscale, 2, s);
  if (band_pixels == 0 || n_views == 0) return ISO_OK;
  ISO_REQUIRE(idx && grad_zbuf && visible, ISO_ERR_INVALID, "iso_splat_band_marks: null pointer");
  ISO_REQUIRE((((uintptr_t)grad_zbuf) & 15) == 0 && ((view_pixels * points_per_pixel) & 3) == 0 &&
                  ((band_pixels * points_per_pixel) & 3) == 0,
              ISO_ERR_UNSUPPORTED, "iso_splat_band_marks: grad_zbuf slices must be 16-byte aligned");
  hipLaunchKernelGGL(k_mark_visible, dim3(iso_stream_grid(band_pixels, 256), n_views), dim3(256), 0, s, idx,
                     points_per_pixel, band_pixels, visible, view_pixels);
  const int64_t n = band_pixels * points_per_pixel;
  int gm = iso_div_up(n, 256 * 16); if (gm > 1024) gm = 1024; if (gm < 1) gm = 1;
  hipLaunchKernelGGL(k_z_absmax, dim3(gm, n_views), dim3(256), 0, s, grad_zbuf, n, reinterpret_cast<ZScale*>(zscale),
                     view_pixels * points_per_pixel);
  ISO_CHECK_LAUNCH("iso_splat_band_marks");
  return ISO_OK;
}

extern "C" int iso_splat_band_z_scatter(const int32_t* idx, const float* grad_zbuf, int n_views, int64_t view_pixels,
                                        int64_t band_pixels, int points_per_pixel, int32_t* zscale, int64_t* acc,
                                        void* stream) {
  ISO_REQUIRE(zscale && acc && n_views >= 0 && view_pixels > 0 && band_pixels >= 0 && points_per_pixel >= 1 &&
                  ((idx && grad_zbuf) || band_pixels == 0),
              ISO_ERR_INVALID, "iso_splat_band_z_scatter: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int terms_log2 = 0;
  while ((1ll << terms_log2) < view_pixels) ++terms_log2;
  hipLaunchKernelGGL(k_z_scale, dim3(1), dim3(1), 0, s, reinterpret_cast<ZScale*>(zscale), terms_log2);
  if (band_pixels > 0 && n_views > 0)
    hipLaunchKernelGGL(k_z_scatter, dim3(iso_stream_grid(band_pixels, 256), n_views), dim3(256), 0, s, idx, grad_zbuf,
                       points_per_pixel, band_pixels, reinterpret_cast<const ZScale*>(zscale),
                       reinterpret_cast<long long*>(acc), view_pixels);
  ISO_CHECK_LAUNCH("iso_splat_band_z_scatter");
  return ISO_OK;
}

namespace {
__global__ void k_z_finish_rows(const long long* __restrict__ acc, const ZScale* __restrict__ zs, int64_t row0, int64_t n,
                                float* __restrict__ grad) {
  const int e = zs->exp2;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const long long a = acc[row0 + j];
    float z = (float)ldexp((double)a, -e);
    if (a >= (1ll << 61) || a <= -(1ll << 61)) z = __builtin_nanf("");
    grad[(row0 + j) * 3 + 2] = z;
  }
}
}  // namespace

extern "C" int iso_splat_z_finish(const int64_t* acc, const int32_t* zscale, int64_t row0, int64_t n_rows,
                                  float* grad_points, void* stream) {
  ISO_REQUIRE(acc && zscale && grad_points && row0 >= 0 && n_rows >= 0, ISO_ERR_INVALID, "iso_splat_z_finish: bad arguments");
  if (n_rows > 0)
    hipLaunchKernelGGL(k_z_finish_rows, dim3(iso_stream_grid(n_rows, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(acc), reinterpret_cast<const ZScale*>(zscale), row0, n_rows,
                       grad_points);
  ISO_CHECK_LAUNCH("iso_splat_z_finish");
  return ISO_OK;
}
