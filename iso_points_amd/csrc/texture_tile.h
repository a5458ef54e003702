// The 64-point tile skeleton of the texture network's tile kernels: k_texture_x16 (texture.hip), its recompute
// k_texgrad_fwd_x16 and the reverse sweep k_texgrad_rev_x16 (texgrad.hip).  One tile is worked by eight waves: the
// activations of its 64 points lie in LDS already cut into two fp16 parts, every wave owns TW output tiles of 32 features
// and streams exactly those weight rows (tex_gemm of texture_gemm.h, three passes per layer), cuts its outputs under the
// next per-point scale into its own K-steps of the activation buffer, and the per-point maxima that bound the next layer
// ride on the barrier that ends the layer.  Tiles are drawn from a counter.
//   tex_forward_tiles<H, STASH>   the whole forward: k_texture_x16 is STASH = false, k_texgrad_fwd_x16 is STASH = true --
//                                 the same rows, scales and GEMMs, every h_l written out, no head
// and the pieces the reverse sweep builds on as well: TexLds, tex_put_amax / tex_get_max, tex_draw_tile / tex_next_tile,
// tex_gemm3, tex_requantize, tex_end_layer, the stash addresses.
#pragma once
#include "texture_gemm.h"

namespace {

constexpr int kTexGeoRows = 48;      // G + V <= 6 + 39
constexpr int kTexP = 64;            // points per tile

struct TexArgs {
  const float* points; const float* normals; const float* codes; const float* origins; const int32_t* origin_of;
  int64_t n_origins;
  float* rgb;
  int64_t n;
  const float* packed;
  TexShape s;
  int32_t* tile_ctr;                 // ZERO when the launch starts: the workgroups draw their next tile from it
};

template <int H>
struct TexTile {
  static constexpr int NW = 8, NB = 2, P = kTexP;
  static constexpr int NS = H / 16, NTO = H / 32, TW = NTO / NW, SL = 2 * TW;
  static constexpr int KSA = NS > kTexK0Max / 16 ? NS : kTexK0Max / 16;       // K-steps the activation buffer holds
  static constexpr size_t kActBytes = (size_t)KSA * NB * kAP * 1024;
  static constexpr size_t kGeoBytes = (size_t)kTexGeoRows * P * sizeof(float);
  static constexpr size_t kRedBytes = (size_t)NW * P * 16;
  static constexpr size_t kLds = kActBytes + kGeoBytes + kRedBytes;
  static_assert(NTO % NW == 0 && TW >= 1, "features must split evenly over the waves");
  static_assert(kLds <= 160 * 1024, "LDS budget");
};

// The register-to-feature map of every stash (x3_feat): registers 8p..8p+7 of the accumulator of output tile T, which is
// also K-step 2 T + p of the next layer's operand, hold features 32 T + 16 p + 4 h + {0..3, 8..11} in lane half h.  The
// offset of the first in a row-major row; the second four lie 8 floats on (tex_store8).
__device__ __forceinline__ int tex_stash_off(int T, int p, int h) { return 32 * T + 16 * p + 4 * h; }

// A thread's view of the tile: where the buffers lie in the dynamic LDS of a tile kernel (launched with TexTile<H>::kLds
// bytes and 512 threads) and the thread's place in the tile.  The buffers are functions, not pointer members: as members
// the compiler no longer knew geo to be LDS where a row entry comes from codes (HBM) or geo, and read both through one
// flat load.
template <int H>
struct TexLds {
  using S = TexTile<H>;
  int tid, w, lane, h, j;            // wave w (uniform), lane = 32 h + j

  static __device__ __forceinline__ unsigned char* base() {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    return smem_raw;
  }
  // [K-step][NB][kAP][64]: the layer's B operand, two fp16 parts per entry
  static __device__ __forceinline__ u32x4* act() { return reinterpret_cast<u32x4*>(base()); }
  // [k][P]: normal, point, view
  static __device__ __forceinline__ float* geo() { return reinterpret_cast<float*>(base() + S::kActBytes); }
  // [NW][P]: the head's partial sums per wave
  static __device__ __forceinline__ f32x4* red() { return reinterpret_cast<f32x4*>(base() + S::kActBytes + S::kGeoBytes); }
  // [2][P][NW]: maxima exchange, the same bytes as red
  static __device__ __forceinline__ float* redm() { return reinterpret_cast<float*>(red()); }
  // this lane's entries of the SL K-steps its wave writes
  __device__ __forceinline__ u32x4* own() const { return act() + (size_t)(S::SL * w) * S::NB * kAP * 64 + lane; }
  // the wave's output tile t is tile T = TW w + t of the layer
  __device__ __forceinline__ int stash_off(int t, int p) const { return tex_stash_off(S::TW * w + t, p, h); }
};

template <int H>
__device__ __forceinline__ TexLds<H> tex_lds() {
  TexLds<H> c;
  c.tid = threadIdx.x;
  c.w = __builtin_amdgcn_readfirstlane(c.tid >> 6);
  c.lane = c.tid & 63; c.h = c.lane >> 5; c.j = c.lane & 31;
  return c;
}

__device__ __forceinline__ void tex_store8(float* dst, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(dst) = (f32x4){v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(dst + 8) = (f32x4){v[4], v[5], v[6], v[7]};
}

// the part of a packed image (texp_fw / tgp_bw) that wave w streams, and the first fragments of its first pass
template <int H>
__device__ __forceinline__ const u32x4* tex_wave_img(const float* img, int w) {
  return reinterpret_cast<const u32x4*>(img) + (TexTile<H>::TW * w * 2) * 64;
}
template <int H>
__device__ __forceinline__ void tex_prefetch_a(u32x4 (&A)[4][TexTile<H>::TW], const u32x4* imgw, int lane) {
#pragma unroll
  for (int d = 0; d < kTexAD; ++d) tex_load_a<TexTile<H>::TW, TexTile<H>::NTO>(A[d], imgw, d, kTexQA[0], lane);
}

// ---- per-point maxima over the waves: every wave puts the maximum of its own features, a barrier, every lane reads all --
template <int H>
__device__ __forceinline__ void tex_put_amax(const TexLds<H>& c, int buf, const float (&amax)[TexTile<H>::NB]) {
  using S = TexTile<H>;
#pragma unroll
  for (int n = 0; n < S::NB; ++n) {
    const float m = __builtin_fmaxf(amax[n], __shfl_xor(amax[n], 32));
    if (c.h == 0) c.redm()[(buf * S::P + 32 * n + c.j) * S::NW + c.w] = m;
  }
}
template <int H>
__device__ __forceinline__ void tex_get_max(const TexLds<H>& c, int buf, float (&Mp)[TexTile<H>::NB]) {
  using S = TexTile<H>;
#pragma unroll
  for (int n = 0; n < S::NB; ++n) {
    float m = 0.f;
#pragma unroll
    for (int ww = 0; ww < S::NW; ++ww) m = __builtin_fmaxf(m, c.redm()[(buf * S::P + 32 * n + c.j) * S::NW + ww]);
    Mp[n] = m;
  }
}

// ---- tiles from the counter: thread 0 asks for the workgroup's next tile when a tile starts (the atomic's latency rides
// under the tile's work) and publishes it when the tile ends.  tex_next_tile is a barrier; the caller follows it with a
// second one before the next tile (the forward's head reduction sits between the two).
__device__ __forceinline__ int tex_draw_tile(int32_t* ctr) {
  int drawn = 0;
  if (threadIdx.x == 0) drawn = (int)gridDim.x + atomicAdd(ctr, 1);
  return drawn;
}
__device__ __forceinline__ int64_t tex_next_tile(int drawn) {
  __shared__ int s_next_tile;
  if (threadIdx.x == 0) s_next_tile = drawn;
  __syncthreads();
  return (int64_t)__builtin_amdgcn_readfirstlane(s_next_tile);               // uniform: the tile's addresses stay scalar
}

// ---- the tile's input rows [ c | normal, point | view ]: their per-point maximum Mp and scale bscale, and the B operand
// of layer 0 in act.  Wave w, lane = point, takes every NW-th geometry row / code column; then the KS0 * NB operand entries
// are spread over the waves, slots above D0 zero.  STASH_X0: the rows go to x0 (n, K0) as well, the B operand of dW_0.
// Two barriers: act, geo and exchange buffer 0 are free on entry, act is complete on return.
template <int H, bool STASH_X0>
__device__ __forceinline__ void tex_assemble_rows(const TexLds<H>& c, const TexArgs& a, int64_t tile, float (&Mp)[TexTile<H>::NB],
                                                  float (&bscale)[TexTile<H>::NB], float* x0) {
  using S = TexTile<H>;
  constexpr int NW = S::NW, NB = S::NB, P = S::P;
  const TexShape& s = a.s;
  const int w = c.w, lane = c.lane, j = c.j, h8 = c.h * 8;
  const int C = s.C, GV = s.G + s.V, KS0 = s.K0 / 16;
  const int64_t count = a.n;
  {
    const int64_t slot = tile * P + lane;
    const bool live = slot < count;
    float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, m = 0.f;
    if (live) {
      px = a.points[slot * 3]; py = a.points[slot * 3 + 1]; pz = a.points[slot * 3 + 2];
      if (s.G == 6) { nx = a.normals[slot * 3]; ny = a.normals[slot * 3 + 1]; nz = a.normals[slot * 3 + 2]; }
      if (s.V > 0) {
        int64_t o = a.origin_of ? (int64_t)a.origin_of[slot] : 0;
        o = o < 0 ? 0 : (o >= a.n_origins ? a.n_origins - 1 : o);
        vx = px - a.origins[o * 3]; vy = py - a.origins[o * 3 + 1]; vz = pz - a.origins[o * 3 + 2];
        // F.normalize: v / max(|v|, 1e-12)
        const float den = __builtin_fmaxf(__builtin_sqrtf((vx * vx + vy * vy) + vz * vz), 1e-12f);
        vx = vx / den; vy = vy / den; vz = vz / den;
      }
      const float* crow = a.codes + slot * C;
#pragma unroll 1
      for (int cc = w; cc < C; cc += NW) m = __builtin_fmaxf(m, __builtin_fabsf(crow[cc]));
    }
#pragma unroll 1
    for (int k = w; k < GV; k += NW) {
      float v = 0.f;
      if (live) {
        if (k < s.G - 3) v = k == 0 ? nx : (k == 1 ? ny : nz);
        else if (k < s.G) { const int cc = k - (s.G - 3); v = cc == 0 ? px : (cc == 1 ? py : pz); }
        else { float dv; int cc; posenc(k - s.G, vx, vy, vz, v, cc, dv); }
      }
      c.geo()[k * P + lane] = v;
      m = __builtin_fmaxf(m, __builtin_fabsf(v));
    }
    c.redm()[(0 * P + lane) * NW + w] = m;
  }
  __syncthreads();
  tex_get_max(c, 0, Mp);
#pragma unroll
  for (int n = 0; n < NB; ++n) bscale[n] = x3_scale_for(Mp[n] * 1.01f);
#pragma unroll 1
  for (int ent = w; ent < KS0 * NB; ent += NW) {
    const int ks = ent / NB, n = ent % NB;
    const int64_t slot = tile * P + 32 * n + j;
    const bool live = slot < count;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int f = x3_feat(ks, h8 + e);
      float x = 0.f;
      if (live && f < C) x = a.codes[slot * C + f];
      else if (f >= C && f < s.D0) x = c.geo()[(f - C) * P + 32 * n + j];
      v[e] = x;
    }
    if constexpr (STASH_X0) {
      if (live) tex_store8(x0 + slot * s.K0 + tex_stash_off(ks >> 1, ks & 1, c.h), v);
    }
    const float sc = n == 0 ? bscale[0] : bscale[1];
    u32x4 p0, p1;
    split8_f16(v, p0, p1, sc);
    c.act()[((ks * NB + n) * kAP + 0) * 64 + lane] = p0;
    c.act()[((ks * NB + n) * kAP + 1) * 64 + lane] = p1;
  }
  __syncthreads();
}

// ---- a layer's GEMM: the three passes of tex_gemm over the wave's rows of `img`, the last one requesting the first
// fragments of `nxt`.  BIAS: acc starts from bias * zs; otherwise the caller has set it.
template <int H, bool BIAS>
__device__ __forceinline__ void tex_gemm3(const TexLds<H>& c, const u32x4* img, const u32x4* nxt,
                                          f32x16 (&acc)[TexTile<H>::TW][TexTile<H>::NB], u32x4 (&A)[4][TexTile<H>::TW],
                                          const float* bias = nullptr, const float* zs = nullptr) {
  using S = TexTile<H>;
  constexpr int NB = S::NB, NS = S::NS, NTO = S::NTO, TW = S::TW;
  tex_gemm<TW, NB, NTO, NS, BIAS>(img, kTexQA[0], c.act() + c.lane, kTexQB[0], acc, 0, A, img, 0, kTexQA[1], c.lane, bias, c.w, zs);
  tex_gemm<TW, NB, NTO, NS, false>(img, kTexQA[1], c.act() + c.lane, kTexQB[1], acc, 0, A, img, 0, kTexQA[2], c.lane);
  tex_gemm<TW, NB, NTO, NS, false>(img, kTexQA[2], c.act() + c.lane, kTexQB[2], acc, 0, A, nxt, 0, kTexQA[0], c.lane);
}

// layer 0: KS0 = K0 / 16 K-steps in groups of four, once per product: every group requests the fragments of the one after it
template <int H>
__device__ __forceinline__ void tex_gemm3_layer0(const TexLds<H>& c, const u32x4* img, const u32x4* nxt, int KS0,
                                                 f32x16 (&acc)[TexTile<H>::TW][TexTile<H>::NB], u32x4 (&A)[4][TexTile<H>::TW],
                                                 const float* bias, const float* zs) {
  using S = TexTile<H>;
  constexpr int NB = S::NB, NTO = S::NTO, TW = S::TW;
  const int NG0 = KS0 / 4;
  for (int g = 0; g < 3 * NG0; ++g) {
    const int q = g / NG0, k0 = 4 * (g % NG0);
    const bool more = g + 1 < 3 * NG0;
    const u32x4* after = more ? img : nxt;
    const int kn = more ? 4 * ((g + 1) % NG0) : 0, pn = more ? kTexQA[(g + 1) / NG0] : kTexQA[0];
    if (g == 0) tex_gemm<TW, NB, NTO, 4, true>(img, kTexQA[q], c.act() + c.lane, kTexQB[q], acc, k0, A, after, kn, pn, c.lane, bias, c.w, zs);
    else tex_gemm<TW, NB, NTO, 4, false>(img, kTexQA[q], c.act() + c.lane, kTexQB[q], acc, k0, A, after, kn, pn, c.lane);
  }
}

// ---- a layer's outputs, eight registers (t, p, n) at a time: f(t, p, n, hv) gives the eight values (from the accumulator,
// with whatever stash traffic goes with them); where they FEED another layer their maximum per point goes to amax (of |hv|
// where SIGNED; f's values are not negative otherwise) and they are cut under nscale into the wave's own K-steps of act.
// Every wave must have read act before (a barrier).  f must inline.
template <int H, bool SIGNED, class F>
__device__ __forceinline__ void tex_requantize(const TexLds<H>& c, const float (&nscale)[TexTile<H>::NB],
                                               float (&amax)[TexTile<H>::NB], bool feed, F&& f) {
  using S = TexTile<H>;
  constexpr int NB = S::NB, TW = S::TW;
#pragma unroll
  for (int n = 0; n < NB; ++n) amax[n] = 0.f;
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const int k = (2 * t + p) * NB + n;
        float hv[8];
        f(t, p, n, hv);
        if (!feed) continue;
        float m = amax[n];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          if constexpr (SIGNED) m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(hv[e]), __builtin_fabsf(hv[e + 1])));
          else m = __builtin_fmaxf(m, __builtin_fmaxf(hv[e], hv[e + 1]));
        }
        amax[n] = m;
        u32x4 p0, p1;
        split8_f16(hv, p0, p1, nscale[n]);
        c.own()[(k * kAP + 0) * 64] = p0; c.own()[(k * kAP + 1) * 64] = p1;
        __builtin_amdgcn_sched_barrier(0);     // one group at a time: bounds register pressure
      }
}

// ---- the end of a layer that feeds another: its scales become the operand's, the maxima are exchanged on the barrier
// after which the next layer's inputs are complete
template <int H>
__device__ __forceinline__ void tex_end_layer(const TexLds<H>& c, int& mbuf, const float (&amax)[TexTile<H>::NB],
                                              const float (&nscale)[TexTile<H>::NB], float (&bscale)[TexTile<H>::NB],
                                              float (&Mp)[TexTile<H>::NB]) {
#pragma unroll
  for (int n = 0; n < TexTile<H>::NB; ++n) bscale[n] = nscale[n];
  mbuf ^= 1;                                   // the exchange buffer written last
  tex_put_amax(c, mbuf, amax);
  __syncthreads();
  tex_get_max(c, mbuf, Mp);
}

// ---- head: three dot products over H from the registers of the top layer (relu(acc / zs)), reduced over the lane halves
// here and over the waves in tex_head_finish (uniform base + 32-bit lane offset, as x3_load_a: no 64-bit per-lane address
// per row)
template <int H>
__device__ __forceinline__ void tex_head_partial(const TexLds<H>& c, const TexArgs& a,
                                                 const f32x16 (&acc)[TexTile<H>::TW][TexTile<H>::NB],
                                                 const float (&zs)[TexTile<H>::NB]) {
  using S = TexTile<H>;
  constexpr int NB = S::NB, TW = S::TW, SL = S::SL, P = S::P;
  typedef const __attribute__((address_space(1))) char* gbytes_t;
  typedef const __attribute__((address_space(1))) f32x4* gf32x4_t;
  const gbytes_t WLu = (gbytes_t)(a.packed + texp_head(a.s) + SL * c.w * 16);
  const unsigned hoff = (unsigned)(c.h * 8) * 4u;
  float fsum[NB][3];
#pragma unroll
  for (int n = 0; n < NB; ++n) fsum[n][0] = fsum[n][1] = fsum[n][2] = 0.f;
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int sl = 2 * t + p;
        const f32x4 wl0 = *(gf32x4_t)(WLu + (ch * H + sl * 16) * 4 + hoff);
        const f32x4 wl1 = *(gf32x4_t)(WLu + (ch * H + sl * 16 + 4) * 4 + hoff);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float iz = 1.0f / zs[n];
          float hv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) hv[e] = __builtin_fmaxf(acc[t][n][8 * p + e] * iz, 0.f);
          fsum[n][ch] += ((wl0.x * hv[0] + wl0.y * hv[1]) + (wl0.z * hv[2] + wl0.w * hv[3])) +
                         ((wl1.x * hv[4] + wl1.y * hv[5]) + (wl1.z * hv[6] + wl1.w * hv[7]));
        }
        __builtin_amdgcn_sched_barrier(0);   // one row's weights at a time: bounds register pressure
      }
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const float r = fsum[n][0] + __shfl_xor(fsum[n][0], 32);
    const float g = fsum[n][1] + __shfl_xor(fsum[n][1], 32);
    const float b = fsum[n][2] + __shfl_xor(fsum[n][2], 32);
    if (c.h == 0) c.red()[c.w * P + 32 * n + c.j] = (f32x4){r, g, b, 0.f};
  }
}

// the three sums over the waves (after a barrier), tanh, (x + 1) / 2
template <int H>
__device__ __forceinline__ void tex_head_finish(const TexLds<H>& c, const TexArgs& a, int64_t tile) {
  using S = TexTile<H>;
  const int tid = c.tid;
  const int64_t slot = tile * S::P + tid;
  if (tid < S::P && slot < a.n) {
    const f32x4 b_head = *reinterpret_cast<const f32x4*>(a.packed + texp_hbias(a.s));
    f32x4 r = c.red()[tid];
#pragma unroll
    for (int ww = 1; ww < S::NW; ++ww) {
      const f32x4 q = c.red()[ww * S::P + tid];
      r.x += q.x; r.y += q.y; r.z += q.z;
    }
    a.rgb[slot * 3] = (tanhf(r.x + b_head.x) + 1.0f) / 2.0f;
    a.rgb[slot * 3 + 1] = (tanhf(r.y + b_head.y) + 1.0f) / 2.0f;
    a.rgb[slot * 3 + 2] = (tanhf(r.z + b_head.z) + 1.0f) / 2.0f;
  }
}

// ---- the forward over the tiles of a launch.  STASH = false is k_texture_x16: the top layer goes through the head to
// a.rgb.  STASH = true is the backward's recompute k_texgrad_fwd_x16: no head; the rows go to x0 (n, K0) and every h_l to
// hst + l * lstride, row-major (n, H).  Everything before the stores is the one code, so the recompute's h_l are the
// forward's bit for bit.
template <int H, bool STASH>
__device__ __forceinline__ void tex_forward_tiles(const TexArgs& a, float* hst = nullptr, int64_t lstride = 0, float* x0 = nullptr) {
  using S = TexTile<H>;
  constexpr int NB = S::NB, TW = S::TW, P = S::P;
  const TexLds<H> c = tex_lds<H>();
  const TexShape s = a.s;
  const int nL = s.n_layers;
  const float* hdr = a.packed;
  auto fwd_img = [&](int l) { return tex_wave_img<H>(a.packed + (l == 0 ? texp_fw0(s) : texp_fw(s, l)), c.w); };
  u32x4 A[4][TW];
  tex_prefetch_a<H>(A, fwd_img(0), c.lane);

  float bscale[NB], amax[NB];
  const int64_t count = a.n;
  const int64_t n_tiles = (count + P - 1) / P;
  int64_t next_tile = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile = next_tile) {
    const int drawn = tex_draw_tile(a.tile_ctr);
    float Mp[NB];
    tex_assemble_rows<H, STASH>(c, a, tile, Mp, bscale, x0);

    f32x16 acc[TW][NB];
    int mbuf = 0;
    for (int l = 0; l < nL; ++l) {
      const u32x4* img = fwd_img(l);
      const float* bias = a.packed + texp_bias(s, l);
      const float wsc = hdr[l];
      float zs[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) zs[n] = wsc * bscale[n];
      const bool top = (l == nL - 1);
      const u32x4* nxt = top ? fwd_img(0) : fwd_img(l + 1);
      if (l == 0) tex_gemm3_layer0<H>(c, img, nxt, s.K0 / 16, acc, A, bias, zs);
      else tex_gemm3<H, true>(c, img, nxt, acc, A, bias, zs);
      __syncthreads();                                   // every wave has read the activations
      if constexpr (!STASH) {
        if (top) { tex_head_partial<H>(c, a, acc, zs); break; }
      }
      // bound of this layer's output per point -> scale of the next operand
      float nscale[NB], iz[NB];
      float* __restrict__ hl = hst + (int64_t)l * lstride;
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        nscale[n] = STASH && top ? 1.0f : x3_scale_for((hdr[16 + l] * Mp[n] + hdr[32 + l]) * 1.01f);
        iz[n] = 1.0f / zs[n];
      }
      tex_requantize<H, false>(c, nscale, amax, !(STASH && top), [&](int t, int p, int n, float (&hv)[8]) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = __builtin_fmaxf(acc[t][n][8 * p + e] * iz[n], 0.f);
        if constexpr (STASH) {
          const int64_t slot = tile * P + 32 * n + c.j;
          if (slot < count) tex_store8(hl + slot * H + c.stash_off(t, p), hv);
        }
      });
      if (STASH && top) break;
      tex_end_layer(c, mbuf, amax, nscale, bscale, Mp);
    }
    next_tile = tex_next_tile(drawn);
    if constexpr (!STASH) tex_head_finish(c, a, tile);
    __syncthreads();
  }
}

}  // namespace
