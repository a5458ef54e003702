// EWA surface splatting for gfx950, stage 4 of 6: the backward pass's search radius, the lower median of the visible
// points' radii by radix select (EllipticalRasterizer.backward, DSS/core/rasterizer.py:884).
#include <float.h>
#include "iso_common.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------- median radius (radix select)
// r_n = lower-median(radii of the visible points of cloud n, both columns) * radii_s
// (rasterizer.py:884; torch.median of the flattened (n,2) tensor).  Radii are >= 0, so their
// f32 bit patterns order like unsigned integers: three histogram passes over digits of 11 + 11 + 10 bits pin
// the k-th key.  Four launches: every pass resolves the digits decided so far from the earlier histograms itself
// (a 2048-bin prefix per workgroup -- cheaper than a launch in between), the last launch resolves all three,
// writes the result and leaves the histograms zeroed, which is the state the workspace must be in on entry.
constexpr int kRselBins = 2048;
constexpr int kRselShift[3] = {21, 10, 0};
constexpr int kRselBits[3] = {11, 11, 10};

// Workgroup-wide (256 lanes): prefix and remaining rank after the first `passes` digits of cloud-local histograms
// h[3][kRselBins].  Returns false when the cloud has no visible value.  All lanes get the same result.
// (pass-major layout hist[3][n_clouds][kRselBins]: one pass's histograms are contiguous -- the N-rank path sums
// exactly that slice over the ranks between two passes)
__device__ bool rsel_resolve(const unsigned* __restrict__ hist, int n, int n_clouds, int passes, unsigned& prefix,
                             long long& k, long long& cnt, long long* s_w /*[4]*/, long long* s_pub /*[2]*/) {
  prefix = 0u; k = 0; cnt = 0;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int q = 0; q < passes; ++q) {
    const unsigned* hq = hist + ((int64_t)q * n_clouds + n) * kRselBins;
    long long v[8], sum = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = hq[t * 8 + e]; sum += v[e]; }
    long long inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { if (j < w) base += s_w[j]; tot += s_w[j]; }
    if (q == 0) { cnt = tot; k = tot > 0 ? (tot - 1) / 2 : 0; }
    if (cnt == 0) { __syncthreads(); return false; }
    long long ex = base + inc - sum;                    // values in the bins before this lane's eight
    if (k >= ex && k < ex + sum) {                      // exactly one lane holds rank k
      int bsel = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) { if (k >= ex + v[e] && e < 7 && bsel == e) { ex += v[e]; bsel = e + 1; } }
      s_pub[0] = t * 8 + bsel; s_pub[1] = ex;
    }
    __syncthreads();
    prefix |= ((unsigned)s_pub[0]) << kRselShift[q];
    k -= s_pub[1];
    __syncthreads();
  }
  return true;
}

template <int PASS>
__global__ __launch_bounds__(256) void k_rsel_hist(const float* __restrict__ radii,
                                                   const uint8_t* __restrict__ visible,
                                                   const int64_t* __restrict__ first,
                                                   const int64_t* __restrict__ num,
                                                   unsigned* __restrict__ hist /*[3][n_clouds][kRselBins]*/) {
  __shared__ unsigned lh[kRselBins];
  __shared__ long long s_w[4], s_pub[2];
  const int n = blockIdx.y, n_clouds = gridDim.y;
  unsigned prefix = 0u;
  long long k, cnt;
  if (PASS > 0 && !rsel_resolve(hist, n, n_clouds, PASS, prefix, k, cnt, s_w, s_pub)) return;
  for (int j = threadIdx.x; j < kRselBins; j += 256) lh[j] = 0u;
  __syncthreads();
  constexpr int shift = kRselShift[PASS];
  constexpr unsigned dmask = (1u << kRselBits[PASS]) - 1u;
  const unsigned hi_mask = PASS == 0 ? 0u : (0xffffffffu << (shift + kRselBits[PASS]));
  const int64_t len = num[n], base = first[n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + i;
    if (!visible[p]) continue;
    const float2 r2 = *reinterpret_cast<const float2*>(radii + p * 2);
    const unsigned k0 = __float_as_uint(r2.x), k1 = __float_as_uint(r2.y);
    if ((k0 & hi_mask) == prefix) atomicAdd(&lh[(k0 >> shift) & dmask], 1u);
    if ((k1 & hi_mask) == prefix) atomicAdd(&lh[(k1 >> shift) & dmask], 1u);
  }
  __syncthreads();
  unsigned* hp = hist + ((int64_t)PASS * n_clouds + n) * kRselBins;
  for (int j = threadIdx.x; j < kRselBins; j += 256)
    if (lh[j]) atomicAdd(&hp[j], lh[j]);
}

// one 256-lane workgroup per cloud: all three digits, the result, and the histograms back to zero
__global__ __launch_bounds__(256) void k_rsel_final(unsigned* __restrict__ hist, int n_clouds, float radii_s,
                                                    float* __restrict__ out) {
  __shared__ long long s_w[4], s_pub[2];
  const int n = blockIdx.x;
  if (n >= n_clouds) return;
  unsigned prefix;
  long long k, cnt;
  const bool any = rsel_resolve(hist, n, n_clouds, 3, prefix, k, cnt, s_w, s_pub);
  if (threadIdx.x == 0) out[n] = any ? __uint_as_float(prefix) * radii_s : 0.0f;
  __syncthreads();
  for (int q = 0; q < 3; ++q)
    for (int j = threadIdx.x; j < kRselBins; j += 256) hist[((int64_t)q * n_clouds + n) * kRselBins + j] = 0u;
}

}  // namespace

// ===========================================================================
extern "C" int64_t iso_splat_median_radius_workspace_bytes(int n_clouds) {
  if (n_clouds < 0) n_clouds = 0;
  return (int64_t)n_clouds * 3 * kRselBins * 4 + 64;
}

extern "C" int iso_splat_median_radius(const float* radii, const uint8_t* visible,
                                       const int64_t* first_idx, const int64_t* num_pts,
                                       int n_clouds, int64_t max_pts, float radii_s,
                                       void* workspace, int64_t workspace_bytes,
                                       float* search_radius_out, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && max_pts >= 0, ISO_ERR_INVALID, "iso_splat_median_radius: bad sizes");
  if (n_clouds == 0) return ISO_OK;
  ISO_REQUIRE(first_idx && num_pts && workspace && search_radius_out && (max_pts == 0 || (radii && visible)),
              ISO_ERR_INVALID, "iso_splat_median_radius: null pointer");
  ISO_REQUIRE(workspace_bytes >= iso_splat_median_radius_workspace_bytes(n_clouds), ISO_ERR_WORKSPACE,
              "iso_splat_median_radius: workspace too small");
  ISO_REQUIRE(((uintptr_t)radii & 7) == 0, ISO_ERR_INVALID, "iso_splat_median_radius: radii must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned* hist = (unsigned*)workspace;      // zero on entry (contract), zero again on exit (k_rsel_final)
  int gx = iso_div_up(max_pts > 0 ? max_pts : 1, 256 * 8);
  if (gx > 512) gx = 512;
  if (max_pts > 0) {
    hipLaunchKernelGGL(k_rsel_hist<0>, dim3(gx, n_clouds), dim3(256), 0, s, radii, visible, first_idx, num_pts, hist);
    hipLaunchKernelGGL(k_rsel_hist<1>, dim3(gx, n_clouds), dim3(256), 0, s, radii, visible, first_idx, num_pts, hist);
    hipLaunchKernelGGL(k_rsel_hist<2>, dim3(gx, n_clouds), dim3(256), 0, s, radii, visible, first_idx, num_pts, hist);
  }
  hipLaunchKernelGGL(k_rsel_final, dim3(n_clouds), dim3(256), 0, s, hist, n_clouds, radii_s, search_radius_out);
  ISO_CHECK_LAUNCH("iso_splat_median_radius");
  return ISO_OK;
}

// The same select in pieces (N ranks: every rank counts its OWN visible rows; the pass's histograms -- the slice
// workspace + pass * n_clouds * 2048 words, n_clouds * 2048 words long -- are summed over the ranks before the next
// piece runs).  pass = 0, 1, 2, then iso_splat_median_final.  Same workspace contract (zero on entry / on exit).
extern "C" int64_t iso_splat_median_pass_words(int n_clouds) { return (int64_t)(n_clouds < 0 ? 0 : n_clouds) * kRselBins; }

extern "C" int iso_splat_median_pass(int pass, const float* radii, const uint8_t* visible, const int64_t* first_idx,
                                     const int64_t* num_pts, int n_clouds, int64_t max_pts, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(pass >= 0 && pass <= 2 && n_clouds >= 0 && max_pts >= 0, ISO_ERR_INVALID, "iso_splat_median_pass: bad arguments");
  if (n_clouds == 0 || max_pts == 0) return ISO_OK;
  ISO_REQUIRE(radii && visible && first_idx && num_pts && workspace, ISO_ERR_INVALID, "iso_splat_median_pass: null pointer");
  ISO_REQUIRE(workspace_bytes >= iso_splat_median_radius_workspace_bytes(n_clouds), ISO_ERR_WORKSPACE,
              "iso_splat_median_pass: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned* hist = (unsigned*)workspace;
  int gx = iso_div_up(max_pts, 256 * 8);
  if (gx > 512) gx = 512;
  if (pass == 0) hipLaunchKernelGGL(k_rsel_hist<0>, dim3(gx, n_clouds), dim3(256), 0, s, radii, visible, first_idx, num_pts, hist);
  else if (pass == 1) hipLaunchKernelGGL(k_rsel_hist<1>, dim3(gx, n_clouds), dim3(256), 0, s, radii, visible, first_idx, num_pts, hist);
  else hipLaunchKernelGGL(k_rsel_hist<2>, dim3(gx, n_clouds), dim3(256), 0, s, radii, visible, first_idx, num_pts, hist);
  ISO_CHECK_LAUNCH("iso_splat_median_pass");
  return ISO_OK;
}

extern "C" int iso_splat_median_final(void* workspace, int n_clouds, float radii_s, float* search_radius_out, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && (n_clouds == 0 || (workspace && search_radius_out)), ISO_ERR_INVALID,
              "iso_splat_median_final: bad arguments");
  if (n_clouds == 0) return ISO_OK;
  hipLaunchKernelGGL(k_rsel_final, dim3(n_clouds), dim3(256), 0, (hipStream_t)stream, (unsigned*)workspace, n_clouds, radii_s,
                     search_radius_out);
  ISO_CHECK_LAUNCH("iso_splat_median_final");
  return ISO_OK;
}
