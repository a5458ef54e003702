// EWA surface splatting for gfx950: the reference's two-stage raster interface, _rasterize_coarse / _rasterize_fine
// (DSS/csrc/rasterize_points.cu:293-441, :503-596).  A compatibility and debugging surface, not the cycle's path (that
// is splat_raster.hip); the pixel's inside test, list epilogue and deep list are the ones of that path (splat_pixel.h).
#include "splat_pixel.h"

#pragma clang fp contract(off)

namespace {

// ---- the reference's two-stage interface: DSS._C._rasterize_coarse / _rasterize_fine (ext.cpp:11-12) --------------
// coarse (RasterizePointsCoarseCudaKernel, rasterize_points.cu:293-441): bin (by, bx) of cloud n -- bin_size x bin_size
// pixels -- lists the PACKED indices of the cloud's points with z >= 0 whose box [p - r, p + r] overlaps the bin's NDC
// extent (PixToNdc of its first / last pixel -+ half a pixel, both comparisons non-strict), -1 behind them.  The
// reference's order inside a bin is the arrival order of its atomics; here: ascending index (the order of the
// reference's CPU path, rasterize_points_cpu.cpp:190-222).  A bin that would hold more than M entries is cut at M and
// *overflow is set (the CUDA reference writes past the bin, its CPU path raises "Got too many points per bin").
// One workgroup per (bin, cloud): it walks the cloud in index order, 256 points a round, and compacts the hits with
// ballots -- the table is a compatibility surface, not the cycle's path (that is the tile lists of k_bin_lds).
__global__ __launch_bounds__(256) void k_coarse_bins(const float* __restrict__ pts, const float* __restrict__ radii,
                                                     const int64_t* __restrict__ first, const int64_t* __restrict__ num,
                                                     int S, int bin_size, int B, int M, int32_t* __restrict__ bin_points,
                                                     int32_t* __restrict__ overflow) {
  __shared__ int s_w[4];
  const int n = blockIdx.y, by = blockIdx.x / B, bx = blockIdx.x % B;
  const float half_pix = 1.0f / (float)S;
  auto pix2ndc = [&](int i) { return -1 + (2 * i + 1.0f) / S; };          // rasterization_utils.cuh:8-11
  const float bx0 = pix2ndc(bx * bin_size) - half_pix, bx1 = pix2ndc((bx + 1) * bin_size - 1) + half_pix;
  const float by0 = pix2ndc(by * bin_size) - half_pix, by1 = pix2ndc((by + 1) * bin_size - 1) + half_pix;
  int32_t* out = bin_points + (((int64_t)n * B + by) * B + bx) * M;
  const int64_t len = num[n], base = first[n];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t filled = 0;
  for (int64_t i0 = 0; i0 < len; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    bool hit = false;
    if (i < len) {
      const int64_t p = base + i;
      const float px = pts[p * 3], py = pts[p * 3 + 1], pz = pts[p * 3 + 2];
      if (!(pz < 0)) {                                                    // :349 (a NaN depth is not "behind")
        const float rx = radii[p * 2], ry = radii[p * 2 + 1];
        const float px0 = px - rx, px1 = px + rx, py0 = py - ry, py1 = py + ry;
        hit = (py0 <= by1) && (by0 <= py1) && (px0 <= bx1) && (bx0 <= px1);   // :366,:378
      }
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (k < w) before += s_w[k]; tot += s_w[k]; }
    if (hit) {
      const int64_t slot = filled + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (slot < M) out[slot] = (int32_t)(base + i);
      else *overflow = 1;
    }
    filled += tot;
    __syncthreads();
  }
  for (int64_t k = (filled < M ? filled : M) + threadIdx.x; k < M; k += 256) out[k] = -1;
}

// fine (RasterizePointsFineCudaKernel, rasterize_points.cu:503-596): every pixel tests the entries of ITS bin (negative
// entries skipped wherever they stand, :567-571) exactly as the naive kernel tests every point (CheckPixelInsidePoint
// :79-97) and keeps the K front-most hits -- by (z, index), the total order of every raster path here; then the
// depth-merging cut and the outputs of k_raster.  One thread per pixel.
struct FinePixel {
  int n, xi, yi;
  float xf, yf;
  const int32_t* bins;     // the M entries of the pixel's bin
  int64_t pix;             // output pixel, flipped in both axes (:577-580)
  __device__ __forceinline__ FinePixel(int64_t pid, const int32_t* __restrict__ bin_points, int B, int M, int bin_size,
                                       const Frame& F) {
    n = (int)(pid / ((int64_t)F.H * F.W));
    yi = (int)((pid / F.W) % F.H); xi = (int)(pid % F.W);
    xf = ndc_x(xi, F); yf = ndc_y(yi, F);
    bins = bin_points + (((int64_t)n * B + yi / bin_size) * B + xi / bin_size) * M;
    pix = ((int64_t)n * F.H + (F.H - 1 - yi)) * F.W + (F.W - 1 - xi);
  }
  // hit(z, p, q) for every entry of the bin that covers the pixel
  template <class Hit>
  __device__ __forceinline__ void walk(const float* __restrict__ pts, const float* __restrict__ ellipse,
                                       const float* __restrict__ cutoff, const float* __restrict__ radii, int M,
                                       int64_t n_points, Hit&& hit) const {
    for (int m = 0; m < M; ++m) {
      const int64_t p = bins[m];
      if (p < 0 || p >= n_points) continue;
      const float pz = pts[p * 3 + 2];
      if (!(pz >= 0.f)) continue;                          // behind the camera (:87-88) or NaN, as every raster path here
      float q;
      if (pixel_inside_point(xf - pts[p * 3], yf - pts[p * 3 + 1], ellipse[p * 3], ellipse[p * 3 + 1], ellipse[p * 3 + 2],
                             radii[p * 2], radii[p * 2 + 1], cutoff[p], q))
        hit(pz, (int)p, q);
    }
  }
};

template <int KMAX>
__global__ __launch_bounds__(256) void k_fine_bins(const float* __restrict__ pts, const float* __restrict__ ellipse,
                                                   const float* __restrict__ cutoff, const float* __restrict__ radii,
                                                   const int32_t* __restrict__ bin_points, int N, int B, int M, int bin_size,
                                                   Frame F, int K, float depth_thres, int64_t n_points,
                                                   int32_t* __restrict__ idx_out, float* __restrict__ zbuf_out,
                                                   float* __restrict__ q_out, float* __restrict__ occ_out) {
  const int64_t npix = (int64_t)N * F.H * F.W;
  for (int64_t pid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pid < npix; pid += (int64_t)gridDim.x * blockDim.x) {
    const FinePixel px(pid, bin_points, B, M, bin_size, F);
    PixK<KMAX> best;
    best.init();
    float wz = FLT_MAX;
    int wi = 0x7fffffff;
    px.walk(pts, ellipse, cutoff, radii, M, n_points, [&](float pz, int p, float q) {
      if (pz < wz || (pz == wz && p < wi)) {
        best.push(pz, p, q, K);
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j == K - 1) { wz = best.z[j]; wi = best.id[j]; }
      }
    });
    write_pixel_lists<KMAX>(best, K, depth_thres, px.pix, idx_out, zbuf_out, q_out, occ_out);
  }
}

// k_fine_bins for points_per_pixel above 32 (the reference's bound is 150, rasterization_utils.cuh:18, checked at
// rasterize_points.cu:246-251): the pixel's list is a DeepList (splat_pixel.h), as in k_raster_deep.  Same walk over the
// bin, same tests, same (z, index) order, same cut.
__global__ __launch_bounds__(256) void k_fine_bins_deep(const float* __restrict__ pts, const float* __restrict__ ellipse,
                                                        const float* __restrict__ cutoff, const float* __restrict__ radii,
                                                        const int32_t* __restrict__ bin_points, int N, int B, int M,
                                                        int bin_size, Frame F, int K, float depth_thres, int64_t n_points,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ zbuf_out,
                                                        float* __restrict__ q_out, float* __restrict__ occ_out) {
  const int64_t npix = (int64_t)N * F.H * F.W;
  for (int64_t pid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pid < npix; pid += (int64_t)gridDim.x * blockDim.x) {
    const FinePixel px(pid, bin_points, B, M, bin_size, F);
    DeepList best(idx_out, zbuf_out, q_out, px.pix, K);
    px.walk(pts, ellipse, cutoff, radii, M, n_points, [&](float pz, int p, float q) { best.push(pz, p, q); });
    best.finish(depth_thres, occ_out, px.pix, nullptr);
  }
}

}  // namespace

// ===========================================================================
extern "C" int iso_rasterize_coarse(const float* points, const float* radii, const int64_t* first_idx,
                                    const int64_t* num_pts, int n_clouds, int image_size, int bin_size,
                                    int max_points_per_bin, int32_t* bin_points_out, int32_t* overflow_out, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && image_size > 0 && bin_size > 0 && max_points_per_bin >= 0, ISO_ERR_INVALID,
              "iso_rasterize_coarse: bad sizes");
  const int B = 1 + (image_size - 1) / bin_size;
  if (n_clouds == 0 || max_points_per_bin == 0) return ISO_OK;
  ISO_REQUIRE(points && radii && first_idx && num_pts && bin_points_out && overflow_out, ISO_ERR_INVALID,
              "iso_rasterize_coarse: null pointer");
  hipLaunchKernelGGL(k_coarse_bins, dim3(B * B, n_clouds), dim3(256), 0, (hipStream_t)stream, points, radii, first_idx,
                     num_pts, image_size, bin_size, B, max_points_per_bin, bin_points_out, overflow_out);
  ISO_CHECK_LAUNCH("iso_rasterize_coarse");
  return ISO_OK;
}

extern "C" int iso_rasterize_fine(const float* points, const float* ellipse, const float* cutoff, const float* radii,
                                  int64_t n_points, const int32_t* bin_points, int n_clouds, int max_points_per_bin,
                                  float depth_merging_thres, int image_size, int bin_size, int points_per_pixel,
                                  int32_t* idx_out, float* zbuf_out, float* qvalue_out, float* occ_out, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && image_size > 0 && bin_size > 0 && max_points_per_bin >= 0 && n_points >= 0, ISO_ERR_INVALID,
              "iso_rasterize_fine: bad sizes");
  ISO_REQUIRE(points_per_pixel >= 1 && points_per_pixel <= 150, ISO_ERR_UNSUPPORTED,
              "iso_rasterize_fine: points_per_pixel must be in [1,150] (rasterization_utils.cuh:18), got %d", points_per_pixel);
  if (n_clouds == 0) return ISO_OK;
  ISO_REQUIRE(idx_out && zbuf_out && qvalue_out && occ_out && (max_points_per_bin == 0 || bin_points) &&
                  (n_points == 0 || (points && ellipse && cutoff && radii)),
              ISO_ERR_INVALID, "iso_rasterize_fine: null pointer");
  const Frame F = make_frame(image_size, image_size);
  const int B = 1 + (image_size - 1) / bin_size;
  const int64_t npix = (int64_t)n_clouds * image_size * image_size;
  const int K = points_per_pixel;
  hipStream_t s = (hipStream_t)stream;
#define ISO_FINE(KM_)                                                                                               \
  hipLaunchKernelGGL(k_fine_bins<KM_>, dim3(iso_stream_grid(npix, 256)), dim3(256), 0, s, points, ellipse, cutoff, radii, \
                     bin_points, n_clouds, B, max_points_per_bin, bin_size, F, K, depth_merging_thres, n_points, idx_out,  \
                     zbuf_out, qvalue_out, occ_out)
  if (K <= 4) ISO_FINE(4);
  else if (K <= 8) ISO_FINE(8);
  else if (K <= 16) ISO_FINE(16);
  else if (K <= 32) ISO_FINE(32);
  else                                          // lists too deep for registers: kept in the output arrays
    hipLaunchKernelGGL(k_fine_bins_deep, dim3(iso_stream_grid(npix, 256)), dim3(256), 0, s, points, ellipse, cutoff, radii,
                       bin_points, n_clouds, B, max_points_per_bin, bin_size, F, K, depth_merging_thres, n_points, idx_out,
                       zbuf_out, qvalue_out, occ_out);
#undef ISO_FINE
  ISO_CHECK_LAUNCH("iso_rasterize_fine");
  return ISO_OK;
}
