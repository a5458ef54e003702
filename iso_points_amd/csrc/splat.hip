// EWA surface splatting for gfx950, stage 1 of 6: visibility flags, the per-point EWA set-up (isotropic, explicit-frame
// and anisotropic variance), the fused filter + compaction + set-up front end and its gradient to the world points.
// (-> splat_raster.hip -> splat_composite.hip; backward: splat_backward.hip, splat_median.hip.)
//
// Reference semantics
//   set-up   : SurfaceSplatting._get_per_point_info and helpers,
//              DSS/core/rasterizer.py:344-563; filter_renderable :184-254
#include <float.h>
#include "iso_common.h"
#include "pca_eig.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float esqrt_arg(float x) {  // eps_sqrt, mathHelper.py:20-25
  float a = fabsf(x);
  return a < 1e-17f ? 1e-17f : a;
}

// ---------------------------------------------------------------- visibility
// flags[n*P+i] = 1 when point i is renderable in view n (rasterizer.py:184-254)
__global__ void k_view_flags(const float* __restrict__ pts, const float* __restrict__ nrm,
                             const float* __restrict__ views, int32_t* __restrict__ flags,
                             int64_t P, float znear, float zfar, int backface) {
  const int n = blockIdx.y;
  const float* V = views + n * 16;  // row-vector convention: p_view = [p,1] @ V
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P;
       i += (int64_t)gridDim.x * blockDim.x) {
    float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    float zv = ((x * V[2] + y * V[6]) + z * V[10]) + V[14];
    bool ok = (zv >= znear) && (zv <= zfar);
    if (backface) {
      float nx = nrm[i * 3], ny = nrm[i * 3 + 1], nz = nrm[i * 3 + 2];
      float nzv = (nx * V[2] + ny * V[6]) + nz * V[10];
      ok = ok && (nzv < 0.f);
    }
    flags[(int64_t)n * P + i] = ok ? 1 : 0;
  }
}

// out[off[e]] = in[e % P] for flagged e (stable: packed order = view-major, point ascending)
__global__ void k_compact_rows(const float* __restrict__ in, const int32_t* __restrict__ flags,
                               const int32_t* __restrict__ off, float* __restrict__ out,
                               int64_t P, int64_t total, int U) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    if (flags[e]) {
      const float* s = in + (e % P) * U;
      float* d = out + (int64_t)off[e] * U;
      for (int u = 0; u < U; ++u) d[u] = s[u];
    }
  }
}

// h = clamp(0.5 * max_{6 nn} d2, 5e-5, 0.01)   (rasterizer.py:375-386)
__global__ void k_vrk_h(const float* __restrict__ dists /*(N,Pmax,7)*/,
                        const int64_t* __restrict__ first, const int64_t* __restrict__ num,
                        const int64_t* __restrict__ cloud_num, float* __restrict__ h, int64_t pmax) {
  const int n = blockIdx.y;
  const int64_t len = num[n];
  const int64_t clen = cloud_num ? cloud_num[n] : len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float* d = dists + ((int64_t)n * pmax + i) * 7;
    float m = -FLT_MAX;
#pragma unroll
    for (int k = 1; k < 7; ++k) {
      float v = (clen < 7) ? 1e-3f : d[k];
      m = fmaxf(m, v);
    }
    float hv = 0.5f * m;
    hv = fminf(fmaxf(hv, 5e-5f), 0.01f);
    h[first[n] + i] = hv;
  }
}

// ---------------------------------------------------------------- per-point EWA set-up
struct SetupOut {
  float* ndc;      // (P,3)
  float* ellipse;  // (P,3)
  float* cutoff;   // (P)
  float* radii;    // (P,2)
  float* scaler;   // (P)
};

// One point in one view (rasterizer.py:344-563; the arithmetic both set-up kernels share).
struct SetupRes { float ndc[3], el[3], rad[2], scaler; };

__device__ __forceinline__ SetupRes splat_setup_point(float x, float y, float z, float nx, float ny, float nz,
                                                      float hk, const float* __restrict__ V,
                                                      const float* __restrict__ M, int S, float sigma,
                                                      float cutoffC) {
  // [p,1] @ M columns 0,1,3 and view depth
  const float xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
  const float yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
  const float t = ((x * M[3] + y * M[7]) + z * M[11]) + M[15];
  const float zv = ((x * V[2] + y * V[6]) + z * V[10]) + V[14];
  const float t2 = iso_eps_denom(t * t, 1e-17f);
  const float td = iso_eps_denom(t, 1e-17f);
  const float j00 = 1.0f / td;
  const float j30 = -1.0f / t2 * xv, j31 = -1.0f / t2 * yv;
  // WJk = M[:3,:] @ Jk  (3x2)
  float w0[3], w1[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    w0[r] = M[r * 4 + 0] * j00 + M[r * 4 + 3] * j30;
    w1[r] = M[r * 4 + 1] * j00 + M[r * 4 + 3] * j31;
  }
  // tangent frame: u0 = normalize(n x (n + e)), u1 = normalize(n x u0), e = axis least
  // aligned with n (a deterministic instance of rasterizer.py:395-397)
  float ex = 0.f, ey = 0.f, ez = 0.f;
  const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
  if (ax <= ay && ax <= az) ex = 1.f; else if (ay <= az) ey = 1.f; else ez = 1.f;
  const float mx = nx + ex, my = ny + ey, mz = nz + ez;
  float ux = ny * mz - nz * my, uy = nz * mx - nx * mz, uz = nx * my - ny * mx;
  float un = sqrtf((ux * ux + uy * uy) + uz * uz);
  un = un > 1e-12f ? un : 1e-12f;
  ux /= un; uy /= un; uz /= un;
  float vx = ny * uz - nz * uy, vy = nz * ux - nx * uz, vz = nx * uy - ny * ux;
  float vn = sqrtf((vx * vx + vy * vy) + vz * vz);
  vn = vn > 1e-12f ? vn : 1e-12f;
  vx /= vn; vy /= vn; vz /= vn;
  // Mk = Sk @ WJk (2x2);  Vk = h * Mk^T Mk
  const float m00 = (ux * w0[0] + uy * w0[1]) + uz * w0[2];
  const float m01 = (ux * w1[0] + uy * w1[1]) + uz * w1[2];
  const float m10 = (vx * w0[0] + vy * w0[1]) + vz * w0[2];
  const float m11 = (vx * w1[0] + vy * w1[1]) + vz * w1[2];
  const float ps = 2.0f / (float)S;
  const float lp = sigma * (ps * ps);
  const float g00 = hk * (m00 * m00 + m10 * m10) + lp;
  const float g01 = hk * (m00 * m01 + m10 * m11);
  const float g11 = hk * (m01 * m01 + m11 * m11) + lp;
  const float detM = m00 * m11 - m01 * m10;
  // det(h M^T M + lp I) = h^2 det(M)^2 + lp h |M|_F^2 + lp^2: all terms positive, so no
  // cancellation (the textbook g00*g11 - g01^2 loses ~cond(G) digits on grazing splats)
  const float fro = (m00 * m00 + m10 * m10) + (m01 * m01 + m11 * m11);
  const float detG = (hk * hk) * (detM * detM) + (lp * hk * fro + lp * lp);
  const float a = g11 / detG, c = g00 / detG, b = (-g01 / detG) + (-g01 / detG);
  // radii (rasterizer.py:514-516: sqrt(4 c cutoff / (4ac - b^2)), sqrt(4 a cutoff / (4ac - b^2))): 4ac - b^2 = 4 / det G,
  // so they are sqrt(g00 cutoff), sqrt(g11 cutoff); the reference's statement subtracts two nearly equal products on
  // grazing splats (4e-4 relative at S = 1040, h = 0.01)
  SetupRes o;
  o.rad[0] = sqrtf(esqrt_arg(g00 * cutoffC));
  o.rad[1] = sqrtf(esqrt_arg(g11 * cutoffC));
  o.scaler = fabsf(detM) / iso_eps_denom(sqrtf(esqrt_arg(detG * 4.0f * 3.14159265358979323846f * 3.14159265358979323846f)), 1e-17f);
  o.ndc[0] = xv / t; o.ndc[1] = yv / t; o.ndc[2] = zv;
  o.el[0] = a; o.el[1] = b; o.el[2] = c;
  return o;
}

// The tangent frame of splat_setup_point, statement for statement, for iso_splat_tangent_frame (the export through which a
// test hands the isotropic kernel's own frame to iso_splat_setup_vrk).  A copy and not a call from splat_setup_point:
// calling it there changed the instruction schedule of k_splat_setup.
__device__ __forceinline__ void splat_tangent_frame(float nx, float ny, float nz, float& ux, float& uy, float& uz,
                                                    float& vx, float& vy, float& vz) {
  // tangent frame: u0 = normalize(n x (n + e)), u1 = normalize(n x u0), e = axis least
  // aligned with n (a deterministic instance of rasterizer.py:395-397)
  float ex = 0.f, ey = 0.f, ez = 0.f;
  const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
  if (ax <= ay && ax <= az) ex = 1.f; else if (ay <= az) ey = 1.f; else ez = 1.f;
  const float mx = nx + ex, my = ny + ey, mz = nz + ez;
  ux = ny * mz - nz * my;
  uy = nz * mx - nx * mz;
  uz = nx * my - ny * mx;
  float un = sqrtf((ux * ux + uy * uy) + uz * uz);
  un = un > 1e-12f ? un : 1e-12f;
  ux /= un; uy /= un; uz /= un;
  vx = ny * uz - nz * uy;
  vy = nz * ux - nx * uz;
  vz = nx * uy - ny * ux;
  float vn = sqrtf((vx * vx + vy * vy) + vz * vz);
  vn = vn > 1e-12f ? vn : 1e-12f;
  vx /= vn; vy /= vn; vz /= vn;
}

__global__ void k_tangent_frame(const float* __restrict__ nrm, int64_t n, float* __restrict__ u, float* __restrict__ v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float ux, uy, uz, vx, vy, vz;
    splat_tangent_frame(nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2], ux, uy, uz, vx, vy, vz);
    u[i * 3] = ux; u[i * 3 + 1] = uy; u[i * 3 + 2] = uz;
    v[i * 3] = vx; v[i * 3 + 1] = vy; v[i * 3 + 2] = vz;
  }
}

// World -> NDC of the point and WJk (3x2), the Jacobian of screen xy with respect to world xyz (_compute_WJk, :441-492):
// the part of the set-up that comes before the local frame (the first lines of splat_setup_point).
struct SetupProj { float xv, yv, t, zv, w0[3], w1[3]; };

__device__ __forceinline__ SetupProj splat_setup_project(float x, float y, float z, const float* __restrict__ V,
                                                         const float* __restrict__ M) {
  SetupProj pj;
  // [p,1] @ M columns 0,1,3 and view depth
  pj.xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
  pj.yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
  pj.t = ((x * M[3] + y * M[7]) + z * M[11]) + M[15];
  pj.zv = ((x * V[2] + y * V[6]) + z * V[10]) + V[14];
  const float t2 = iso_eps_denom(pj.t * pj.t, 1e-17f);
  const float td = iso_eps_denom(pj.t, 1e-17f);
  const float j00 = 1.0f / td;
  const float j30 = -1.0f / t2 * pj.xv, j31 = -1.0f / t2 * pj.yv;
  // WJk = M[:3,:] @ Jk  (3x2)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    pj.w0[r] = M[r * 4 + 0] * j00 + M[r * 4 + 3] * j30;
    pj.w1[r] = M[r * 4 + 1] * j00 + M[r * 4 + 3] * j31;
  }
  return pj;
}

// The part after the frame for an explicit frame and two variances: Sk = [u; v] (2x3) spans the splat's plane, Vrk = c1 u u^T + c2 v v^T
// is its source-space variance.  Mk = Sk @ WJk, G = Mk^T diag(c1, c2) Mk + lp I; ellipse, radii and scaler follow from G and
// |det Mk| (:499-563), the general form of _compute_anisotropic_Vrk (:257-291).  splat_setup_point above is the instance
// c1 == c2 = h with the frame derived from the normal and G = h Mk^T Mk + lp I factored; it is kept as it was (splitting it
// changed the instruction schedule of the isotropic kernels), and this sibling falls back to the factored form by select
// where the two variances of a row are equal, so an isotropic row gives the same bits through either entry.  Every output
// is even in u and in v: the eigensolver's arbitrary signs do not matter.
__device__ __forceinline__ SetupRes splat_setup_frame(const SetupProj& pj, float ux, float uy, float uz, float vx, float vy,
                                                      float vz, float c1, float c2, int S, float sigma, float cutoffC) {
  const float* w0 = pj.w0;
  const float* w1 = pj.w1;
  // Mk = Sk @ WJk (2x2)
  const float m00 = (ux * w0[0] + uy * w0[1]) + uz * w0[2];
  const float m01 = (ux * w1[0] + uy * w1[1]) + uz * w1[2];
  const float m10 = (vx * w0[0] + vy * w0[1]) + vz * w0[2];
  const float m11 = (vx * w1[0] + vy * w1[1]) + vz * w1[2];
  const float ps = 2.0f / (float)S;
  const float lp = sigma * (ps * ps);
  const float hk = c1;
  // Vk = h * Mk^T Mk
  float g00 = hk * (m00 * m00 + m10 * m10) + lp;
  float g01 = hk * (m00 * m01 + m10 * m11);
  float g11 = hk * (m01 * m01 + m11 * m11) + lp;
  const float detM = m00 * m11 - m01 * m10;
  // det(h M^T M + lp I) = h^2 det(M)^2 + lp h |M|_F^2 + lp^2: all terms positive, so no
  // cancellation (the textbook g00*g11 - g01^2 loses ~cond(G) digits on grazing splats)
  const float fro = (m00 * m00 + m10 * m10) + (m01 * m01 + m11 * m11);
  float detG = (hk * hk) * (detM * detM) + (lp * hk * fro + lp * lp);
  {
    // det(G) = c1 c2 det(Mk)^2 + lp (c1 |row0(Mk)|^2 + c2 |row1(Mk)|^2) + lp^2: the same expansion, all terms non-negative
    const bool same = c1 == c2;
    const float a00 = (c1 * (m00 * m00) + c2 * (m10 * m10)) + lp;
    const float a01 = c1 * (m00 * m01) + c2 * (m10 * m11);
    const float a11 = (c1 * (m01 * m01) + c2 * (m11 * m11)) + lp;
    const float adet = (c1 * c2) * (detM * detM) +
                       (lp * (c1 * (m00 * m00 + m01 * m01) + c2 * (m10 * m10 + m11 * m11)) + lp * lp);
    g00 = same ? g00 : a00;
    g01 = same ? g01 : a01;
    g11 = same ? g11 : a11;
    detG = same ? detG : adet;
  }
  const float a = g11 / detG, c = g00 / detG, b = (-g01 / detG) + (-g01 / detG);
  // radii = sqrt(g00 cutoff), sqrt(g11 cutoff): see splat_setup_point
  SetupRes o;
  o.rad[0] = sqrtf(esqrt_arg(g00 * cutoffC));
  o.rad[1] = sqrtf(esqrt_arg(g11 * cutoffC));
  o.scaler = fabsf(detM) / iso_eps_denom(sqrtf(esqrt_arg(detG * 4.0f * 3.14159265358979323846f * 3.14159265358979323846f)), 1e-17f);
  o.ndc[0] = pj.xv / pj.t; o.ndc[1] = pj.yv / pj.t; o.ndc[2] = pj.zv;
  o.el[0] = a; o.el[1] = b; o.el[2] = c;
  return o;
}

__global__ void k_splat_setup(const float* __restrict__ pts, const float* __restrict__ nrm,
                              const float* __restrict__ h, const int64_t* __restrict__ first,
                              const int64_t* __restrict__ num, const float* __restrict__ views,
                              const float* __restrict__ projs, int S, float sigma, float cutoffC,
                              SetupOut o) {
  const int n = blockIdx.y;
  const float* V = views + n * 16;
  const float* M = projs + n * 16;  // full world->NDC, row-vector convention
  const int64_t len = num[n], base = first[n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + i;
    const SetupRes r = splat_setup_point(pts[p * 3], pts[p * 3 + 1], pts[p * 3 + 2], nrm[p * 3], nrm[p * 3 + 1],
                                         nrm[p * 3 + 2], h[p], V, M, S, sigma, cutoffC);
    o.ndc[p * 3] = r.ndc[0]; o.ndc[p * 3 + 1] = r.ndc[1]; o.ndc[p * 3 + 2] = r.ndc[2];
    o.ellipse[p * 3] = r.el[0]; o.ellipse[p * 3 + 1] = r.el[1]; o.ellipse[p * 3 + 2] = r.el[2];
    o.cutoff[p] = cutoffC;
    o.radii[p * 2] = r.rad[0]; o.radii[p * 2 + 1] = r.rad[1];
    o.scaler[p] = r.scaler;
  }
}

// The set-up for an explicit local frame: frames (P,3,3) packed, eigenvector c in column c, curvature (P,3) ascending
// (what iso_pca_frames writes); the two larger eigenpairs span the splat (rasterizer.py:281-290).
__global__ void k_splat_setup_vrk(const float* __restrict__ pts, const float* __restrict__ frames,
                                  const float* __restrict__ curv, const int64_t* __restrict__ first,
                                  const int64_t* __restrict__ num, const float* __restrict__ views,
                                  const float* __restrict__ projs, int S, float sigma, float cutoffC, SetupOut o) {
  const int n = blockIdx.y;
  const float* V = views + n * 16;
  const float* M = projs + n * 16;
  const int64_t len = num[n], base = first[n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + i;
    const float* f = frames + p * 9;
    const SetupProj pj = splat_setup_project(pts[p * 3], pts[p * 3 + 1], pts[p * 3 + 2], V, M);
    const SetupRes r = splat_setup_frame(pj, f[1], f[4], f[7], f[2], f[5], f[8], curv[p * 3 + 1], curv[p * 3 + 2], S, sigma,
                                         cutoffC);
    o.ndc[p * 3] = r.ndc[0]; o.ndc[p * 3 + 1] = r.ndc[1]; o.ndc[p * 3 + 2] = r.ndc[2];
    o.ellipse[p * 3] = r.el[0]; o.ellipse[p * 3 + 1] = r.el[1]; o.ellipse[p * 3 + 2] = r.el[2];
    o.cutoff[p] = cutoffC;
    o.radii[p * 2] = r.rad[0]; o.radii[p * 2 + 1] = r.rad[1];
    o.scaler[p] = r.scaler;
  }
}

// Anisotropic set-up, fused: one lane per packed row gathers its 8 neighbours of the SAME view cloud through the kNN
// index (N, p_stride, 8; indices local to the cloud), solves the neighbourhood covariance with the device code of
// k_pca_frames (pca_eig.h) and goes straight into the set-up; the frame never reaches memory.
constexpr int kVrkK = 8;       // neighborhood_size of _compute_anisotropic_Vrk (rasterizer.py:275)
__global__ void __launch_bounds__(256) k_splat_setup_aniso(const float* __restrict__ pts, const int64_t* __restrict__ idx,
                                                           int64_t p_stride, const int64_t* __restrict__ first,
                                                           const int64_t* __restrict__ num,
                                                           const float* __restrict__ views,
                                                           const float* __restrict__ projs, int S, float sigma,
                                                           float cutoffC, SetupOut o) {
  const int n = blockIdx.y;
  const float* V = views + n * 16;
  const float* M = projs + n * 16;
  const int64_t base = first[n];
  const int64_t len = min(num[n], p_stride);
  const float* cloud = pts + base * 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + i;
    float l[3], v[3][3];
    pca_neighbourhood_eig(cloud, idx + ((int64_t)n * p_stride + i) * kVrkK, kVrkK, len, l, v);
    const SetupProj pj = splat_setup_project(pts[p * 3], pts[p * 3 + 1], pts[p * 3 + 2], V, M);
    const SetupRes r = splat_setup_frame(pj, v[0][1], v[1][1], v[2][1], v[0][2], v[1][2], v[2][2], l[1], l[2], S, sigma,
                                         cutoffC);
    o.ndc[p * 3] = r.ndc[0]; o.ndc[p * 3 + 1] = r.ndc[1]; o.ndc[p * 3 + 2] = r.ndc[2];
    o.ellipse[p * 3] = r.el[0]; o.ellipse[p * 3 + 1] = r.el[1]; o.ellipse[p * 3 + 2] = r.el[2];
    o.cutoff[p] = cutoffC;
    o.radii[p * 2] = r.rad[0]; o.radii[p * 2 + 1] = r.rad[1];
    o.scaler[p] = r.scaler;
  }
}

// Invariant mode (_compute_global_Vrk, rasterizer.py:293-342): ONE h per cloud = clamp(mean_i 0.5 * max_{6 nn} d2, 5e-5,
// 1e-3).  The reference's mean runs over the PADDED (N, padded_len, 6) tensor of ALL clouds of its call (padded_len = the
// largest one's length, given by the caller, who may hand the clouds over in several calls): it divides by padded_len,
// and a row past a shorter cloud's length contributes what the neighbour search padded it with (-1 from FRNN: -0.5); a
// cloud of fewer than 7 points has every row, padded ones included, set to 1e-3.  Deterministic: workgroup (s, n) adds
// slice s of cloud n in double and a fixed-shape tree in LDS, the finish adds the slices in order.
constexpr int kHSlices = 64;
constexpr int kHBlock = 256;
__global__ void __launch_bounds__(kHBlock) k_vrk_h_partial(const float* __restrict__ dists /*(N,p_stride,7)*/,
                                                           const int64_t* __restrict__ num, int64_t p_stride, int64_t pmax,
                                                           double* __restrict__ part) {
  __shared__ double s_sum[kHBlock];
  const int n = blockIdx.y, s = blockIdx.x;
  const int64_t clen = num[n];
  const int64_t len = min(max(clen, (int64_t)0), p_stride);    // rows of `dists` that exist for this cloud
  const int64_t chunk = (pmax + kHSlices - 1) / kHSlices;
  const int64_t lo = s * chunk, hi = min(lo + chunk, pmax);
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kHBlock) {
    float m = -1.0f;                                           // a padded row: FRNN's fill
    if (clen < 7) {
      m = 1e-3f;
    } else if (i < len) {
      const float* d = dists + ((int64_t)n * p_stride + i) * 7;
      m = -FLT_MAX;
#pragma unroll
      for (int k = 1; k < 7; ++k) m = fmaxf(m, d[k]);
    }
    acc += (double)(0.5f * m);
  }
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kHBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(int64_t)n * kHSlices + s] = s_sum[0];
}

__global__ void __launch_bounds__(256) k_vrk_h_finish(const double* __restrict__ part, const int64_t* __restrict__ first,
                                                      const int64_t* __restrict__ num, int64_t pmax,
                                                      float* __restrict__ h) {
  __shared__ float s_h;
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int s = 0; s < kHSlices; ++s) acc += part[(int64_t)n * kHSlices + s];
    const float mean = (float)(acc / (double)(pmax > 0 ? pmax : 1));
    s_h = fminf(fmaxf(mean, 5e-5f), 1e-3f);
  }
  __syncthreads();
  const float hv = s_h;
  const int64_t len = num[n], base = first[n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x)
    h[base + i] = hv;
}

// ---------------------------------------------------------------- fused filter + compaction + set-up
// The cycle's front end works on the UNFILTERED cloud: a point's renderable views are bits of
// mask[i] (iso_splat_view_mask), its bandwidths h[v*P+i] (iso_splat_h_fused).  The packed order of
// the reference (view-major, points ascending: rasterizer.py:597-618) needs, for point i in view v,
// the number of renderable points before it: chunk counts (k_mask_chunk_count) -> one scan
// (k_mask_chunk_scan, also first_idx / num_points on the device: no host read anywhere) -> ranks
// inside the chunk from wave ballots here.
constexpr int kChunk = 1024;   // points per workgroup: 256 lanes x 4 consecutive points

__global__ __launch_bounds__(256) void k_mask_chunk_count(const int32_t* __restrict__ mask, int64_t P, int n_views,
                                                          int n_chunks, int32_t* __restrict__ chunk_cnt /*(8, n_chunks)*/) {
  __shared__ int s_cnt[8];
  if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kChunk + threadIdx.x * 4;
  int m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = i0 + k < P ? mask[i0 + k] : 0;
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    if (v < n_views) {
      int c = ((m[0] >> v) & 1) + ((m[1] >> v) & 1) + ((m[2] >> v) & 1) + ((m[3] >> v) & 1);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[v], c);
    }
  }
  __syncthreads();
  if (threadIdx.x < n_views) chunk_cnt[threadIdx.x * n_chunks + blockIdx.x] = s_cnt[threadIdx.x];
}

// ---- renderable flags of every point for up to 8 views (rasterizer.py:184-254) --------------------
// (the bit-mask form of k_view_flags: what the fused bandwidth kernel of bricks_h.hip reads)
__global__ __launch_bounds__(256) void k_view_mask(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                   const float* __restrict__ views, int n_views, int64_t n,
                                                   float znear, float zfar, int backface,
                                                   int32_t* __restrict__ mask, int32_t* __restrict__ view_count) {
  __shared__ int s_cnt[8];
  if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  int local[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (backface) { nx = nrm[i * 3]; ny = nrm[i * 3 + 1]; nz = nrm[i * 3 + 2]; }
    int m = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if (v < n_views) {
        const float* V = views + v * 16;                    // row-vector convention: p_view = [p,1] @ V
        const float zv = ((x * V[2] + y * V[6]) + z * V[10]) + V[14];
        bool ok = (zv >= znear) && (zv <= zfar);
        if (backface) ok = ok && (((nx * V[2] + ny * V[6]) + nz * V[10]) < 0.f);
        if (ok) { m |= 1 << v; ++local[v]; }
      }
    }
    mask[i] = m;
  }
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    if (v < n_views) {
      int c = local[v];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[v], c);
    }
  }
  __syncthreads();
  if (threadIdx.x < n_views && s_cnt[threadIdx.x]) atomicAdd(&view_count[threadIdx.x], s_cnt[threadIdx.x]);
}

// The renderable mask of rasterizer.py:184-254 (k_view_mask above: same expressions) AND the chunk counts
// in one pass: a workgroup owns the kChunk consecutive points the front end's workgroup of the same index will own.
__global__ __launch_bounds__(256) void k_view_mask_chunks(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                          const float* __restrict__ views, int n_views, int64_t P,
                                                          float znear, float zfar, int backface, int n_chunks,
                                                          int32_t* __restrict__ mask, int32_t* __restrict__ chunk_cnt) {
  __shared__ int s_cnt[8];
  if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kChunk + threadIdx.x * 4;
  int local[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = i0 + k;
    if (i >= P) break;
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (backface) { nx = nrm[i * 3]; ny = nrm[i * 3 + 1]; nz = nrm[i * 3 + 2]; }
    int m = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if (v < n_views) {
        const float* V = views + v * 16;                    // row-vector convention: p_view = [p,1] @ V
        const float zv = ((x * V[2] + y * V[6]) + z * V[10]) + V[14];
        bool ok = (zv >= znear) && (zv <= zfar);
        if (backface) ok = ok && (((nx * V[2] + ny * V[6]) + nz * V[10]) < 0.f);
        if (ok) { m |= 1 << v; ++local[v]; }
      }
    }
    mask[i] = m;
  }
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    if (v < n_views) {
      int c = local[v];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[v], c);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n_views) chunk_cnt[threadIdx.x * n_chunks + blockIdx.x] = s_cnt[threadIdx.x];
}

// one workgroup: exclusive scan of every view's chunk counts in place; first_idx / num_points (i64,
// the layout _C.splat_points takes) and the int32 view totals
__global__ __launch_bounds__(1024) void k_mask_chunk_scan(int32_t* __restrict__ chunk_cnt, int n_chunks, int n_views,
                                                         int64_t* __restrict__ first, int64_t* __restrict__ num,
                                                         int32_t* __restrict__ view_total) {
  __shared__ int s_w[16];
  __shared__ int s_tot[8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int v = 0; v < n_views; ++v) {
    int carry = 0;
    int32_t* row = chunk_cnt + (int64_t)v * n_chunks;
    for (int c0 = 0; c0 < n_chunks; c0 += 1024) {
      const int i = c0 + threadIdx.x;
      const int val = i < n_chunks ? row[i] : 0;
      int inc = val;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
      if (lane == 63) s_w[w] = inc;
      __syncthreads();
      int base = 0, tot = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) { const int sv = s_w[k]; if (k < w) base += sv; tot += sv; }
      if (i < n_chunks) row[i] = carry + base + inc - val;
      carry += tot;
      __syncthreads();
    }
    if (threadIdx.x == 0) s_tot[v] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int v = 0; v < n_views; ++v) { first[v] = run; num[v] = s_tot[v]; view_total[v] = s_tot[v]; run += s_tot[v]; }
    for (int v = n_views; v < 8; ++v) view_total[v] = 0;
  }
}

struct FrontOut {
  float* ndc; float* ellipse; float* cutoff; float* radii; float* scaler;
  float* feat;      // (cap, C) packed features or null
  int32_t* src;     // (cap) original point of a packed row, or null
  uint8_t* vis0;    // (cap) "visible" flags of the backward pass, cleared here row by row (or null): no fill launch
  int64_t cap;      // rows the arrays hold (<= 0: whatever comes); rows beyond are dropped and *overflow is set
  int32_t* overflow;
};

__global__ __launch_bounds__(256) void k_splat_front(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                     const float* __restrict__ feat_in, int C,
                                                     const int32_t* __restrict__ mask, const float* __restrict__ h,
                                                     int64_t P, const int32_t* __restrict__ chunk_off, int n_chunks,
                                                     const int64_t* __restrict__ first, const float* __restrict__ views,
                                                     const float* __restrict__ projs, int n_views, int S, float sigma,
                                                     float cutoffC, int feat_from_normal, FrontOut o) {
  __shared__ int s_w[8][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kChunk + threadIdx.x * 4;
  int m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = i0 + k < P ? mask[i0 + k] : 0;
  // rank of my first point among the chunk's renderable points, per view
  int rank[8];
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    rank[v] = 0;
    if (v < n_views) {
      const int c = ((m[0] >> v) & 1) + ((m[1] >> v) & 1) + ((m[2] >> v) & 1) + ((m[3] >> v) & 1);
      int inc = c;
#pragma unroll
      for (int o2 = 1; o2 < 64; o2 <<= 1) { const int t = __shfl_up(inc, o2); if (lane >= o2) inc += t; }
      if (lane == 63) s_w[v][w] = inc;
      rank[v] = inc - c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 8; ++v)
    if (v < n_views)
      for (int k = 0; k < w; ++k) rank[v] += s_w[v][k];
  // The rows of a chunk in one view are contiguous in the packed arrays: they are staged in LDS view by view and
  // written out as full lines (a lane storing its own 12-byte rows touches every 128-byte line three times: 350 MB
  // of partial writes for 168 MB of records at 1 M points x 4 views).
  __shared__ float s_ndc[kChunk * 3], s_el[kChunk * 3], s_rad[kChunk * 2], s_sc[kChunk], s_ft[kChunk * 3];
  __shared__ int s_src[kChunk];
  const bool any = (m[0] | m[1] | m[2] | m[3]) != 0;
  float x[4], y[4], z[4], nx[4], ny[4], nz[4], f[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x[k] = y[k] = z[k] = nx[k] = ny[k] = nz[k] = 0.f;
    f[k][0] = f[k][1] = f[k][2] = 0.f;
    if (!m[k]) continue;
    const int64_t i = i0 + k;
    x[k] = pts[i * 3]; y[k] = pts[i * 3 + 1]; z[k] = pts[i * 3 + 2];
    nx[k] = nrm[i * 3]; ny[k] = nrm[i * 3 + 1]; nz[k] = nrm[i * 3 + 2];
    if (o.feat && feat_from_normal) {               // 0.5 (normalize(n) + 1): the cycle's shading-free features
      float nn = sqrtf((nx[k] * nx[k] + ny[k] * ny[k]) + nz[k] * nz[k]);
      nn = nn > 1e-12f ? nn : 1e-12f;
      f[k][0] = 0.5f * (nx[k] / nn + 1.0f); f[k][1] = 0.5f * (ny[k] / nn + 1.0f); f[k][2] = 0.5f * (nz[k] / nn + 1.0f);
    } else if (o.feat && C <= 3) {
      for (int c = 0; c < C; ++c) f[k][c] = feat_in[i * C + c];
    }
  }
  const bool stage_feat = o.feat && C <= 3;         // wider feature rows are written directly
  const int Cs = C;
  for (int v = 0; v < n_views; ++v) {
    const int cnt = s_w[v][0] + s_w[v][1] + s_w[v][2] + s_w[v][3];
    if (cnt == 0) continue;                                                      // workgroup-uniform
    const int64_t p0 = first[v] + chunk_off[(int64_t)v * n_chunks + blockIdx.x];
    int wcnt = cnt;                                       // rows of this chunk and view that fit the arrays
    if (o.cap > 0 && p0 + cnt > o.cap) {
      wcnt = p0 < o.cap ? (int)(o.cap - p0) : 0;
      if (threadIdx.x == 0 && o.overflow) *o.overflow = 1;
    }
    int lr = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q == v) lr = rank[q];
    if (any) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!((m[k] >> v) & 1)) continue;
        const int64_t i = i0 + k;
        const SetupRes r = splat_setup_point(x[k], y[k], z[k], nx[k], ny[k], nz[k], h[(int64_t)v * P + i], views + v * 16,
                                             projs + v * 16, S, sigma, cutoffC);
        s_ndc[lr * 3] = r.ndc[0]; s_ndc[lr * 3 + 1] = r.ndc[1]; s_ndc[lr * 3 + 2] = r.ndc[2];
        s_el[lr * 3] = r.el[0]; s_el[lr * 3 + 1] = r.el[1]; s_el[lr * 3 + 2] = r.el[2];
        s_rad[lr * 2] = r.rad[0]; s_rad[lr * 2 + 1] = r.rad[1];
        s_sc[lr] = r.scaler;
        s_src[lr] = (int32_t)i;
        if (stage_feat)
          for (int c = 0; c < Cs; ++c) s_ft[lr * Cs + c] = f[k][c];
        else if (o.feat && lr < wcnt)
          for (int c = 0; c < C; ++c)
            o.feat[(p0 + lr) * C + c] = feat_from_normal ? (c < 3 ? f[k][c] : 0.f) : feat_in[i * C + c];
        ++lr;
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < wcnt * 3; j += 256) {
      o.ndc[p0 * 3 + j] = s_ndc[j];
      o.ellipse[p0 * 3 + j] = s_el[j];
    }
    for (int j = threadIdx.x; j < wcnt * 2; j += 256) o.radii[p0 * 2 + j] = s_rad[j];
    for (int j = threadIdx.x; j < wcnt; j += 256) {
      o.cutoff[p0 + j] = cutoffC;
      o.scaler[p0 + j] = s_sc[j];
      if (o.src) o.src[p0 + j] = s_src[j];
      if (o.vis0) o.vis0[p0 + j] = 0;
    }
    if (stage_feat)
      for (int j = threadIdx.x; j < wcnt * Cs; j += 256) o.feat[p0 * Cs + j] = s_ft[j];
    __syncthreads();
  }
}

}  // namespace

// ===========================================================================
extern "C" int iso_splat_view_flags(const float* points, const float* normals,
                                    const float* views, int32_t* flags, int64_t P, int n_views,
                                    float znear, float zfar, int backface_culling, void* stream) {
  ISO_REQUIRE(P >= 0 && n_views >= 0, ISO_ERR_INVALID, "iso_splat_view_flags: bad sizes");
  if (P == 0 || n_views == 0) return ISO_OK;
  ISO_REQUIRE(points && views && flags && (normals || !backface_culling), ISO_ERR_INVALID,
              "iso_splat_view_flags: null pointer");
  int gx = iso_div_up(P, 256); if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(k_view_flags, dim3(gx, n_views), dim3(256), 0, (hipStream_t)stream, points,
                     normals, views, flags, P, znear, zfar, backface_culling);
  ISO_CHECK_LAUNCH("iso_splat_view_flags");
  return ISO_OK;
}

extern "C" int iso_compact_rows(const float* in, const int32_t* flags, const int32_t* offsets,
                                float* out, int64_t P, int64_t total, int U, void* stream) {
  ISO_REQUIRE(P >= 0 && total >= 0 && U >= 0, ISO_ERR_INVALID, "iso_compact_rows: bad sizes");
  if (total == 0 || U == 0) return ISO_OK;
  ISO_REQUIRE(in && flags && offsets && out && P > 0, ISO_ERR_INVALID, "iso_compact_rows: null pointer");
  hipLaunchKernelGGL(k_compact_rows, dim3(iso_stream_grid(total, 256)), dim3(256), 0,
                     (hipStream_t)stream, in, flags, offsets, out, P, total, U);
  ISO_CHECK_LAUNCH("iso_compact_rows");
  return ISO_OK;
}

extern "C" int iso_splat_vrk_h(const float* dists, const int64_t* first_idx, const int64_t* num_pts,
                               const int64_t* cloud_num_pts, float* h, int n_clouds,
                               int64_t p_stride, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && p_stride >= 0, ISO_ERR_INVALID, "iso_splat_vrk_h: bad sizes");
  if (n_clouds == 0 || p_stride == 0) return ISO_OK;
  ISO_REQUIRE(dists && first_idx && num_pts && h, ISO_ERR_INVALID, "iso_splat_vrk_h: null pointer");
  int gx = iso_div_up(p_stride, 256); if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(k_vrk_h, dim3(gx, n_clouds), dim3(256), 0, (hipStream_t)stream, dists,
                     first_idx, num_pts, cloud_num_pts, h, p_stride);
  ISO_CHECK_LAUNCH("iso_splat_vrk_h");
  return ISO_OK;
}

extern "C" int iso_splat_setup(const float* points, const float* normals, const float* h,
                               const int64_t* first_idx, const int64_t* num_pts,
                               const float* views, const float* projs, int n_views,
                               int64_t max_pts, int image_size, float sigma, float cutoff,
                               float* ndc_out, float* ellipse_out, float* cutoff_out,
                               float* radii_out, float* scaler_out, void* stream) {
  ISO_REQUIRE(n_views >= 0 && max_pts >= 0 && image_size > 0, ISO_ERR_INVALID, "iso_splat_setup: bad sizes");
  if (n_views == 0 || max_pts == 0) return ISO_OK;
  ISO_REQUIRE(points && normals && h && first_idx && num_pts && views && projs && ndc_out &&
                  ellipse_out && cutoff_out && radii_out && scaler_out,
              ISO_ERR_INVALID, "iso_splat_setup: null pointer");
  SetupOut o{ndc_out, ellipse_out, cutoff_out, radii_out, scaler_out};
  int gx = iso_div_up(max_pts, 256); if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(k_splat_setup, dim3(gx, n_views), dim3(256), 0, (hipStream_t)stream, points,
                     normals, h, first_idx, num_pts, views, projs, image_size, sigma, cutoff, o);
  ISO_CHECK_LAUNCH("iso_splat_setup");
  return ISO_OK;
}

extern "C" int64_t iso_splat_vrk_h_global_work_bytes(int n_clouds) {
  return n_clouds > 0 ? (int64_t)n_clouds * kHSlices * (int64_t)sizeof(double) : 0;
}

extern "C" int iso_splat_vrk_h_global(const float* dists, const int64_t* first_idx, const int64_t* num_pts, float* h,
                                      int n_clouds, int64_t p_stride, int64_t padded_len, void* work, void* stream) {
  ISO_REQUIRE(n_clouds >= 0 && p_stride >= 0 && padded_len >= p_stride, ISO_ERR_INVALID,
              "iso_splat_vrk_h_global: bad sizes (padded_len must be >= p_stride)");
  if (n_clouds == 0 || p_stride == 0) return ISO_OK;
  ISO_REQUIRE(dists && first_idx && num_pts && h && work, ISO_ERR_INVALID, "iso_splat_vrk_h_global: null pointer");
  hipLaunchKernelGGL(k_vrk_h_partial, dim3(kHSlices, n_clouds), dim3(kHBlock), 0, (hipStream_t)stream, dists, num_pts,
                     p_stride, padded_len, (double*)work);
  ISO_CHECK_LAUNCH("iso_splat_vrk_h_global (partial sums)");
  int gx = iso_div_up(p_stride, 256); if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(k_vrk_h_finish, dim3(gx, n_clouds), dim3(256), 0, (hipStream_t)stream, (const double*)work, first_idx,
                     num_pts, padded_len, h);
  ISO_CHECK_LAUNCH("iso_splat_vrk_h_global");
  return ISO_OK;
}

extern "C" int iso_splat_tangent_frame(const float* normals, int64_t n, float* u_out, float* v_out, void* stream) {
  ISO_REQUIRE(n >= 0, ISO_ERR_INVALID, "iso_splat_tangent_frame: bad sizes");
  if (n == 0) return ISO_OK;
  ISO_REQUIRE(normals && u_out && v_out, ISO_ERR_INVALID, "iso_splat_tangent_frame: null pointer");
  hipLaunchKernelGGL(k_tangent_frame, dim3(iso_stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, normals, n, u_out,
                     v_out);
  ISO_CHECK_LAUNCH("iso_splat_tangent_frame");
  return ISO_OK;
}

extern "C" int iso_splat_setup_vrk(const float* points, const float* frames, const float* curvature,
                                   const int64_t* first_idx, const int64_t* num_pts, const float* views, const float* projs,
                                   int n_views, int64_t max_pts, int image_size, float sigma, float cutoff, float* ndc_out,
                                   float* ellipse_out, float* cutoff_out, float* radii_out, float* scaler_out, void* stream) {
  ISO_REQUIRE(n_views >= 0 && max_pts >= 0 && image_size > 0, ISO_ERR_INVALID, "iso_splat_setup_vrk: bad sizes");
  if (n_views == 0 || max_pts == 0) return ISO_OK;
  ISO_REQUIRE(points && frames && curvature && first_idx && num_pts && views && projs && ndc_out && ellipse_out &&
                  cutoff_out && radii_out && scaler_out,
              ISO_ERR_INVALID, "iso_splat_setup_vrk: null pointer");
  SetupOut o{ndc_out, ellipse_out, cutoff_out, radii_out, scaler_out};
  int gx = iso_div_up(max_pts, 256); if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(k_splat_setup_vrk, dim3(gx, n_views), dim3(256), 0, (hipStream_t)stream, points, frames, curvature,
                     first_idx, num_pts, views, projs, image_size, sigma, cutoff, o);
  ISO_CHECK_LAUNCH("iso_splat_setup_vrk");
  return ISO_OK;
}

extern "C" int iso_splat_setup_aniso(const float* points, const int64_t* knn_idx, int64_t p_stride,
                                     const int64_t* first_idx, const int64_t* num_pts, const float* views,
                                     const float* projs, int n_views, int image_size, float sigma, float cutoff,
                                     float* ndc_out, float* ellipse_out, float* cutoff_out, float* radii_out,
                                     float* scaler_out, void* stream) {
  ISO_REQUIRE(n_views >= 0 && p_stride >= 0 && image_size > 0, ISO_ERR_INVALID, "iso_splat_setup_aniso: bad sizes");
  if (n_views == 0 || p_stride == 0) return ISO_OK;
  ISO_REQUIRE(points && knn_idx && first_idx && num_pts && views && projs && ndc_out && ellipse_out && cutoff_out &&
                  radii_out && scaler_out,
              ISO_ERR_INVALID, "iso_splat_setup_aniso: null pointer");
  SetupOut o{ndc_out, ellipse_out, cutoff_out, radii_out, scaler_out};
  int gx = iso_div_up(p_stride, 256); if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(k_splat_setup_aniso, dim3(gx, n_views), dim3(256), 0, (hipStream_t)stream, points, knn_idx, p_stride,
                     first_idx, num_pts, views, projs, image_size, sigma, cutoff, o);
  ISO_CHECK_LAUNCH("iso_splat_setup_aniso");
  return ISO_OK;
}

extern "C" int64_t iso_splat_front_workspace_bytes(int64_t n_points) {
  if (n_points < 0) n_points = 0;
  // [chunk table 8 x (n_chunks + 1) ints][per-tile counts 8 x (4 n_chunks + 4) ints: filled by a projection launch with
  //  iso_follow, scanned into the chunk table by iso_bricks_build_pending]
  const int64_t n_chunks = (n_points + kChunk - 1) / kChunk;
  return 8 * 4 * (n_chunks + 1) + 8 * 4 * (4 * n_chunks + 4);
}

// ---- gradient of the packed NDC rows w.r.t. the world points ---------------------------------------
// Row (v, i) of the front end is ndc = (xv / t, yv / t, zv) with [xv, yv, ., t] = [p, 1] M_v and zv = [p, 1] V_v[:, 2]
// (splat_setup_point; SurfaceSplatting.transform, rasterizer.py:565-582 -> cameras.transform_points), so
//   d L / d p_j = sum_v  gx (M[j][0] - ndc_x M[j][3]) / t + gy (M[j][1] - ndc_y M[j][3]) / t + gz V[j][2].
// Point-major: thread = point, views in ascending order (deterministic); the row of (v, i) is found by binary
// search in the view's ascending src list.
__global__ void k_splat_points_backward(const float* __restrict__ pts, int64_t n, const float* __restrict__ views,
                                        const float* __restrict__ projs, int n_views, const int32_t* __restrict__ mask,
                                        const int32_t* __restrict__ src, const int64_t* __restrict__ first,
                                        const int64_t* __restrict__ num, const float* __restrict__ grad_ndc,
                                        float* __restrict__ grad_pts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    const int m = mask[i];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int v = 0; v < n_views; ++v) {
      if (!((m >> v) & 1)) continue;
      const int32_t* sv = src + first[v];
      int64_t lo = 0, hi = num[v];
      while (lo < hi) {                       // first row whose source point is >= i
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sv[mid] < i) lo = mid + 1; else hi = mid;
      }
      if (lo >= num[v] || (int64_t)sv[lo] != i) continue;      // (cannot happen for a mask / src pair of one front end)
      const int64_t row = first[v] + lo;
      const float* M = projs + v * 16;
      const float* V = views + v * 16;
      const float xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
      const float yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
      const float t = ((x * M[3] + y * M[7]) + z * M[11]) + M[15];
      const float it = 1.0f / iso_eps_denom(t, 1e-17f);
      const float nx = xv * it, ny = yv * it;
      const float g0 = grad_ndc[row * 3] * it, g1 = grad_ndc[row * 3 + 1] * it, g2 = grad_ndc[row * 3 + 2];
      gx += (g0 * (M[0] - nx * M[3]) + g1 * (M[1] - ny * M[3])) + g2 * V[2];
      gy += (g0 * (M[4] - nx * M[7]) + g1 * (M[5] - ny * M[7])) + g2 * V[6];
      gz += (g0 * (M[8] - nx * M[11]) + g1 * (M[9] - ny * M[11])) + g2 * V[10];
    }
    grad_pts[i * 3] = gx; grad_pts[i * 3 + 1] = gy; grad_pts[i * 3 + 2] = gz;
  }
}

extern "C" int iso_splat_points_backward(const float* points, int64_t n_points, const float* views, const float* projs,
                                         int n_views, const int32_t* mask, const int32_t* src, const int64_t* first_idx,
                                         const int64_t* num_points, const float* grad_ndc, float* grad_points,
                                         void* stream) {
  ISO_REQUIRE(n_points >= 0 && n_views >= 1 && n_views <= 8, ISO_ERR_INVALID, "iso_splat_points_backward: bad sizes (1..8 views)");
  if (n_points == 0) return ISO_OK;
  ISO_REQUIRE(points && views && projs && mask && src && first_idx && num_points && grad_ndc && grad_points, ISO_ERR_INVALID,
              "iso_splat_points_backward: null pointer");
  hipLaunchKernelGGL(k_splat_points_backward, dim3(iso_stream_grid(n_points, 256)), dim3(256), 0, (hipStream_t)stream, points,
                     n_points, views, projs, n_views, mask, src, first_idx, num_points, grad_ndc, grad_points);
  ISO_CHECK_LAUNCH("iso_splat_points_backward");
  return ISO_OK;
}

extern "C" int iso_splat_front(const float* points, const float* normals, const float* features, int channels,
                               int features_from_normals, const int32_t* mask, const float* h, int64_t n_points,
                               const float* views, const float* projs, int n_views, int image_size, float sigma,
                               float cutoff, void* workspace, int64_t workspace_bytes, int64_t* first_idx_out,
                               int64_t* num_pts_out, int32_t* view_total_out, float* ndc_out, float* ellipse_out,
                               float* cutoff_out, float* radii_out, float* scaler_out, float* features_out,
                               int32_t* src_out, void* stream) {
  ISO_REQUIRE(n_points >= 0 && n_views >= 1 && n_views <= 8 && image_size > 0, ISO_ERR_INVALID,
              "iso_splat_front: bad sizes (1..8 views per call)");
  ISO_REQUIRE(channels >= 0 && channels <= 8, ISO_ERR_UNSUPPORTED, "iso_splat_front: channels must be <= 8");
  ISO_REQUIRE(!features_from_normals || channels == 3, ISO_ERR_INVALID, "iso_splat_front: features_from_normals needs 3 channels");
  ISO_REQUIRE(first_idx_out && num_pts_out && view_total_out && workspace, ISO_ERR_INVALID, "iso_splat_front: null pointer");
  ISO_REQUIRE(workspace_bytes >= iso_splat_front_workspace_bytes(n_points), ISO_ERR_WORKSPACE,
              "iso_splat_front: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int n_chunks = (int)((n_points + kChunk - 1) / kChunk);
  int32_t* chunk = (int32_t*)workspace;
  if (n_points > 0) {
    ISO_REQUIRE(points && normals && mask && h && views && projs && ndc_out && ellipse_out && cutoff_out && radii_out &&
                    scaler_out && (!features_out || features || features_from_normals),
                ISO_ERR_INVALID, "iso_splat_front: null pointer");
    hipLaunchKernelGGL(k_mask_chunk_count, dim3(n_chunks), dim3(256), 0, s, mask, n_points, n_views, n_chunks, chunk);
  }
  hipLaunchKernelGGL(k_mask_chunk_scan, dim3(1), dim3(1024), 0, s, chunk, n_chunks, n_views, first_idx_out, num_pts_out,
                     view_total_out);
  if (n_points > 0) {
    FrontOut o{ndc_out, ellipse_out, cutoff_out, radii_out, scaler_out, features_out, src_out, nullptr, 0, nullptr};
    hipLaunchKernelGGL(k_splat_front, dim3(n_chunks), dim3(256), 0, s, points, normals, features, channels, mask, h,
                       n_points, chunk, n_chunks, first_idx_out, views, projs, n_views, image_size, sigma, cutoff,
                       features_from_normals, o);
  }
  ISO_CHECK_LAUNCH("iso_splat_front");
  return ISO_OK;
}

extern "C" int iso_splat_view_mask(const float* points, const float* normals, const float* views, int n_views,
                                   int64_t n, float znear, float zfar, int backface_culling, int32_t* mask_out,
                                   int32_t* view_count_out, void* stream) {
  ISO_REQUIRE(n >= 0 && n_views >= 1 && n_views <= 8, ISO_ERR_UNSUPPORTED, "iso_splat_view_mask: 1..8 views per call");
  ISO_REQUIRE(views && mask_out && view_count_out && (points || n == 0) && (normals || !backface_culling),
              ISO_ERR_INVALID, "iso_splat_view_mask: null pointer");
  hipStream_t s = (hipStream_t)stream;
  iso_zero_words(view_count_out, 8, s);
  if (n > 0)
    hipLaunchKernelGGL(k_view_mask, dim3(iso_stream_grid(n, 256 * 4)), dim3(256), 0, s, points, normals, views, n_views,
                       n, znear, zfar, backface_culling, mask_out, view_count_out);
  ISO_CHECK_LAUNCH("iso_splat_view_mask");
  return ISO_OK;
}

// The renderable mask, its per-chunk counts and their scan in two launches: what iso_splat_view_mask +
// the first two launches of iso_splat_front do in five.  The workspace (iso_splat_front_workspace_bytes) then holds
// the scanned chunk table iso_splat_front_rows expects; first_idx / num_points / view_total are final.
extern "C" int iso_splat_view_mask_scan(const float* points, const float* normals, const float* views, int n_views,
                                        int64_t n_points, float znear, float zfar, int backface_culling,
                                        int32_t* mask_out, void* workspace, int64_t workspace_bytes,
                                        int64_t* first_idx_out, int64_t* num_pts_out, int32_t* view_total_out,
                                        void* stream) {
  ISO_REQUIRE(n_points >= 0 && n_views >= 1 && n_views <= 8, ISO_ERR_UNSUPPORTED, "iso_splat_view_mask_scan: 1..8 views per call");
  ISO_REQUIRE(views && workspace && first_idx_out && num_pts_out && view_total_out &&
                  (n_points == 0 || (points && mask_out && (normals || !backface_culling))),
              ISO_ERR_INVALID, "iso_splat_view_mask_scan: null pointer");
  ISO_REQUIRE(workspace_bytes >= iso_splat_front_workspace_bytes(n_points), ISO_ERR_WORKSPACE,
              "iso_splat_view_mask_scan: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int n_chunks = (int)((n_points + kChunk - 1) / kChunk);
  int32_t* chunk = (int32_t*)workspace;
  if (n_points > 0)
    hipLaunchKernelGGL(k_view_mask_chunks, dim3(n_chunks), dim3(256), 0, s, points, normals, views, n_views, n_points, znear,
                       zfar, backface_culling, n_chunks, mask_out, chunk);
  hipLaunchKernelGGL(k_mask_chunk_scan, dim3(1), dim3(1024), 0, s, chunk, n_chunks, n_views, first_idx_out, num_pts_out,
                     view_total_out);
  ISO_CHECK_LAUNCH("iso_splat_view_mask_scan");
  return ISO_OK;
}

// iso_splat_front after iso_splat_view_mask_scan: the compaction + set-up pass alone (one launch); workspace,
// first_idx and mask are the ones that call produced.
extern "C" int iso_splat_front_rows(const float* points, const float* normals, const float* features, int channels,
                                    int features_from_normals, const int32_t* mask, const float* h, int64_t n_points,
                                    const float* views, const float* projs, int n_views, int image_size, float sigma,
                                    float cutoff, const void* workspace, int64_t workspace_bytes, const int64_t* first_idx,
                                    float* ndc_out, float* ellipse_out, float* cutoff_out, float* radii_out,
                                    float* scaler_out, float* features_out, int32_t* src_out, uint8_t* visible_zero_out,
                                    int64_t row_capacity, int32_t* overflow_out, void* stream) {
  ISO_REQUIRE(n_points >= 0 && n_views >= 1 && n_views <= 8 && image_size > 0, ISO_ERR_INVALID,
              "iso_splat_front_rows: bad sizes (1..8 views per call)");
  ISO_REQUIRE(channels >= 0 && channels <= 8, ISO_ERR_UNSUPPORTED, "iso_splat_front_rows: channels must be <= 8");
  ISO_REQUIRE(!features_from_normals || channels == 3, ISO_ERR_INVALID, "iso_splat_front_rows: features_from_normals needs 3 channels");
  ISO_REQUIRE(first_idx && workspace && workspace_bytes >= iso_splat_front_workspace_bytes(n_points), ISO_ERR_INVALID,
              "iso_splat_front_rows: workspace / first_idx missing");
  if (n_points == 0) return ISO_OK;
  ISO_REQUIRE(points && normals && mask && h && views && projs && ndc_out && ellipse_out && cutoff_out && radii_out &&
                  scaler_out && (!features_out || features || features_from_normals),
              ISO_ERR_INVALID, "iso_splat_front_rows: null pointer");
  const int n_chunks = (int)((n_points + kChunk - 1) / kChunk);
  FrontOut o{ndc_out, ellipse_out, cutoff_out, radii_out, scaler_out, features_out, src_out, visible_zero_out, row_capacity, overflow_out};
  hipLaunchKernelGGL(k_splat_front, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, points, normals, features, channels,
                     mask, h, n_points, (const int32_t*)workspace, n_chunks, first_idx, views, projs, n_views, image_size,
                     sigma, cutoff, features_from_normals, o);
  ISO_CHECK_LAUNCH("iso_splat_front_rows");
  return ISO_OK;
}
