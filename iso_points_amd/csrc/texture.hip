// Texture network (RenderingNetwork, DSS/models/common.py:313-366, fed as NeuralTexture.forward builds its rows,
// DSS/core/texture.py:136-162) on the fp16 matrix cores at f32 accuracy, forward only: the value-only form of
// idr_x16.hip (activations of one 64-point tile in LDS already cut into two fp16 parts, every wave owns its output
// features and streams exactly those weight rows, three partial products per layer accumulated in f32, two barriers per
// layer, tiles drawn from a counter) with
//  * the layer GEMM in three passes over K (tex_gemm below): the two small partial products first, the large one on top;
//  * layer 0 a GEMM over the input row [ c (C) | normal, point (G) | view (V) ], D0 = C + G + V <= 301, K padded to a
//    multiple of 64: the B operand is assembled per tile -- the code row read from HBM, normal / point read once, the view
//    direction normalize(p - origin) encoded with posenc() of idr_common.h -- and no (n, D0) matrix exists in HBM;
//  * ReLU instead of softplus: the bound of a layer's output per point is rowsum_l * max_k |h_{l-1}[k][p]| + max |b_l| (no
//    ln2 / beta term), and the INPUT row carries a per-point scale as well, because codes are not bounded by 1;
//  * three head rows, tanh, (x + 1) / 2.
//   c     = codes[i]                                              (n, C)
//   x     = [c, normal_i, p_i, e(normalize(p_i - origin[origin_of[i]]))]
//   h_0   = relu(W_0 x + b_0),  h_l = relu(W_l h_{l-1} + b_l),  rgb = (tanh(W_n h_{n-1} + b_n) + 1) / 2
#include "idr_common.h"
#include "mfma_split.h"
#include "texture_common.h"
#include "texture_gemm.h"

namespace {

// kernel code: 600 + hidden / 16 = k_texture_x16<hidden>; -1: refused (tex_shape_ok of texture_common.h)
int tex_form(int H, int n_layers, int C, int G, int F) { return tex_shape_ok(H, n_layers, C, G, F) ? 600 + H / 16 : -1; }

// per layer: 2^s_l with max |2^s_l W_l| in [512, 1024), the largest row sum of |W_l| and the largest |b_l|
__global__ void k_texture_stats(const float* __restrict__ raw, float* __restrict__ packed, TexShape s) {
  __shared__ float s_m[256];
  const int H = s.H, l = blockIdx.x;
  auto block_max = [&](float v) {
    s_m[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) s_m[threadIdx.x] = fmaxf(s_m[threadIdx.x], s_m[threadIdx.x + o]);
      __syncthreads();
    }
    const float r = s_m[0];
    __syncthreads();
    return r;
  };
  const float* __restrict__ Wl = raw + tex_raw_off(s, l);
  const int nb = tex_in_dim(s, l);
  float mx = 0.f, rs = 0.f, bm = 0.f;
  for (int a = threadIdx.x; a < H; a += 256) {
    const float* __restrict__ row = Wl + (int64_t)a * nb;
    float t = 0.f;
    for (int b0 = 0; b0 < nb; b0 += 32) {
      float v[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) v[q] = fabsf(row[min(b0 + q, nb - 1)]);
#pragma unroll
      for (int q = 0; q < 32; ++q) { const float u = b0 + q < nb ? v[q] : 0.f; t += u; mx = fmaxf(mx, u); }
    }
    rs = fmaxf(rs, t);
    bm = fmaxf(bm, fabsf(Wl[(int64_t)H * nb + a]));
  }
  mx = block_max(mx); rs = block_max(rs); bm = block_max(bm);
  if (threadIdx.x == 0) {
    float sc = 1.0f;
    if (mx > 0.f && mx < 3.0e38f) {
      int e;
      (void)frexpf(mx, &e);
      int k = 10 - e;                          // 2^k * mx in [512, 1024)
      k = k > 100 ? 100 : (k < -100 ? -100 : k);
      sc = ldexpf(1.0f, k);
    }
    packed[l] = sc; packed[16 + l] = rs; packed[32 + l] = bm;
  }
}

__global__ void k_texture_pack(const float* __restrict__ raw, float* __restrict__ packed, TexShape s) {
  const int H = s.H, nL = s.n_layers, NTO = H / 32;
  const int64_t HH = (int64_t)H * H;
  const int64_t b0 = texp_bias(s, 0), e0 = texp_end(s);
  for (int64_t o = b0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < e0; o += (int64_t)gridDim.x * blockDim.x) {
    if (o < texp_head(s)) {                                      // biases, K-order
      const int l = (int)((o - b0) / H);
      packed[o] = raw[tex_raw_off(s, l) + (int64_t)H * tex_in_dim(s, l) + tex_feat_of_ko((o - b0) % H)];
    } else if (o < texp_hbias(s)) {                              // head rows, K-order
      const int64_t q = o - texp_head(s);
      packed[o] = raw[tex_raw_off(s, nL) + (q / H) * H + tex_feat_of_ko(q % H)];
    } else if (o < texp_fw0(s)) {                                // head bias, one pad
      const int c = (int)(o - texp_hbias(s));
      packed[o] = c < 3 ? raw[tex_raw_off(s, nL) + 3 * (int64_t)H + c] : 0.f;
    } else {                                                     // fp16 images: one 32-bit word = two halves
      int l = 0;
      int64_t q = o - texp_fw0(s);
      if (o >= texp_fw(s, 1)) {
        const int64_t r = o - texp_fw(s, 1);
        l = 1 + (int)(r / HH);
        q = r % HH;
      }
      const float sc = packed[l];                                // written by k_texture_stats, the launch before
      const int nb = tex_in_dim(s, l);
      const int d = (int)(q & 3), lane = (int)((q >> 2) & 63);
      const int64_t blk = q >> 8;                                // (ks*NTO + To)*2 + part
      const int part = (int)(blk & 1);
      const int To = (int)((blk >> 1) % NTO), ks = (int)(blk / (2 * NTO));
      const int fo = 32 * To + (lane & 31);
      f32x2 v;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int fi = x3_feat(ks, 8 * (lane >> 5) + 2 * d + u);
        v[u] = fi < nb ? raw[tex_raw_off(s, l) + (int64_t)fo * nb + fi] * sc : 0.f;
      }
      const f16x2 h = __builtin_convertvector(v, f16x2);
      const f16x2 lo = __builtin_convertvector(v - __builtin_convertvector(h, f32x2), f16x2);
      reinterpret_cast<unsigned*>(packed)[o] = part == 0 ? __builtin_bit_cast(unsigned, h) : __builtin_bit_cast(unsigned, lo);
    }
  }
}

template <int H>
__global__ __launch_bounds__(512, 1) void k_texture_x16(TexArgs a) {
  using S = TexTile<H>;
  constexpr int NW = S::NW, NB = S::NB, NS = S::NS, NTO = S::NTO, TW = S::TW, SL = S::SL, P = S::P;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* act = reinterpret_cast<u32x4*>(smem_raw);
  float* geo = reinterpret_cast<float*>(smem_raw + S::kActBytes);                    // [k][P]: normal, point, view
  f32x4* red = reinterpret_cast<f32x4*>(smem_raw + S::kActBytes + S::kGeoBytes);     // [NW][P]
  float* redm = reinterpret_cast<float*>(red);                                      // [2][P][NW] maxima exchange
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, h = lane >> 5, j = lane & 31, h8 = h * 8;
  const TexShape s = a.s;
  const int nL = s.n_layers, C = s.C, GV = s.G + s.V, KS0 = s.K0 / 16;
  const float* hdr = a.packed;
  u32x4* own = act + (size_t)(SL * w) * NB * kAP * 64 + lane;

  auto fwd_img = [&](int l) {
    const float* base = a.packed + (l == 0 ? texp_fw0(s) : texp_fw(s, l));
    return reinterpret_cast<const u32x4*>(base) + (TW * w * 2) * 64;
  };
  u32x4 A[4][TW];
#pragma unroll
  for (int d = 0; d < kTexAD; ++d) tex_load_a<TW, NTO>(A[d], fwd_img(0), d, kTexQA[0], lane);

  float bscale[NB], amax[NB];
  auto put_amax = [&](int buf) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const float m = __builtin_fmaxf(amax[n], __shfl_xor(amax[n], 32));
      if (h == 0) redm[(buf * P + 32 * n + j) * NW + w] = m;
    }
  };
  auto get_max = [&](int buf, float (&Mp)[NB]) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float m = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) m = __builtin_fmaxf(m, redm[(buf * P + 32 * n + j) * NW + ww]);
      Mp[n] = m;
    }
  };

  const int64_t count = a.n;
  const int64_t n_tiles = (count + P - 1) / P;
  __shared__ int s_next_tile;
  int64_t next_tile = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile = next_tile) {
    int drawn = 0;
    if (tid == 0) drawn = (int)gridDim.x + atomicAdd(a.tile_ctr, 1);
    // ---- the row's geometry part and its largest entry: wave w, lane = point, takes every NW-th row / code column --
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
        for (int c = w; c < C; c += NW) m = __builtin_fmaxf(m, __builtin_fabsf(crow[c]));
      }
#pragma unroll 1
      for (int k = w; k < GV; k += NW) {
        float v = 0.f;
        if (live) {
          if (k < s.G - 3) v = k == 0 ? nx : (k == 1 ? ny : nz);
          else if (k < s.G) { const int c = k - (s.G - 3); v = c == 0 ? px : (c == 1 ? py : pz); }
          else { float dv; int c; posenc(k - s.G, vx, vy, vz, v, c, dv); }
        }
        geo[k * P + lane] = v;
        m = __builtin_fmaxf(m, __builtin_fabsf(v));
      }
      redm[(0 * P + lane) * NW + w] = m;
    }
    __syncthreads();
    float Mp[NB];
    get_max(0, Mp);
#pragma unroll
    for (int n = 0; n < NB; ++n) bscale[n] = x3_scale_for(Mp[n] * 1.01f);
    // B operand of layer 0: the KS0*NB entries are spread over the waves; slots above D0 are zero
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
        else if (f >= C && f < s.D0) x = geo[(f - C) * P + 32 * n + j];
        v[e] = x;
      }
      const float sc = n == 0 ? bscale[0] : bscale[1];
      u32x4 p0, p1;
      split8_f16(v, p0, p1, sc);
      act[((ks * NB + n) * kAP + 0) * 64 + lane] = p0;
      act[((ks * NB + n) * kAP + 1) * 64 + lane] = p1;
    }
    __syncthreads();

    f32x16 acc[TW][NB];
    int mbuf = 0;                              // exchange buffer written last
    for (int l = 0; l < nL; ++l) {
      const u32x4* img = fwd_img(l);
      const float* bias = a.packed + texp_bias(s, l);
      const float wsc = hdr[l];
      float zs[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) zs[n] = wsc * bscale[n];
      const bool top = (l == nL - 1);
      const u32x4* nxt = top ? fwd_img(0) : fwd_img(l + 1);
      if (l == 0) {
        // K0 / 16 K-steps in groups of four, once per product: every group requests the fragments of the one after it
        const int NG0 = KS0 / 4;
        for (int g = 0; g < 3 * NG0; ++g) {
          const int q = g / NG0, k0 = 4 * (g % NG0);
          const bool more = g + 1 < 3 * NG0;
          const u32x4* after = more ? img : nxt;
          const int kn = more ? 4 * ((g + 1) % NG0) : 0, pn = more ? kTexQA[(g + 1) / NG0] : kTexQA[0];
          if (g == 0) tex_gemm<TW, NB, NTO, 4, true>(img, kTexQA[q], act + lane, kTexQB[q], acc, k0, A, after, kn, pn, lane, bias, w, zs);
          else tex_gemm<TW, NB, NTO, 4, false>(img, kTexQA[q], act + lane, kTexQB[q], acc, k0, A, after, kn, pn, lane);
        }
      } else {
        tex_gemm<TW, NB, NTO, NS, true>(img, kTexQA[0], act + lane, kTexQB[0], acc, 0, A, img, 0, kTexQA[1], lane, bias, w, zs);
        tex_gemm<TW, NB, NTO, NS, false>(img, kTexQA[1], act + lane, kTexQB[1], acc, 0, A, img, 0, kTexQA[2], lane);
        tex_gemm<TW, NB, NTO, NS, false>(img, kTexQA[2], act + lane, kTexQB[2], acc, 0, A, nxt, 0, kTexQA[0], lane);
      }
      __syncthreads();                                   // every wave has read the activations
      if (top) {
        // ---- head: three dot products over H from the registers, reduced over the lane halves here and over the waves below
        // (uniform base + 32-bit lane offset, as x3_load_a: no 64-bit per-lane address per row)
        typedef const __attribute__((address_space(1))) char* gbytes_t;
        typedef const __attribute__((address_space(1))) f32x4* gf32x4_t;
        const gbytes_t WLu = (gbytes_t)(a.packed + texp_head(s) + SL * w * 16);
        const unsigned hoff = (unsigned)h8 * 4u;
        float fsum[NB][3];
#pragma unroll
        for (int n = 0; n < NB; ++n) fsum[n][0] = fsum[n][1] = fsum[n][2] = 0.f;
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int sl = 2 * t + p;
              const f32x4 wl0 = *(gf32x4_t)(WLu + (c * H + sl * 16) * 4 + hoff);
              const f32x4 wl1 = *(gf32x4_t)(WLu + (c * H + sl * 16 + 4) * 4 + hoff);
#pragma unroll
              for (int n = 0; n < NB; ++n) {
                const float iz = 1.0f / zs[n];
                float hv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = __builtin_fmaxf(acc[t][n][8 * p + e] * iz, 0.f);
                fsum[n][c] += ((wl0.x * hv[0] + wl0.y * hv[1]) + (wl0.z * hv[2] + wl0.w * hv[3])) +
                              ((wl1.x * hv[4] + wl1.y * hv[5]) + (wl1.z * hv[6] + wl1.w * hv[7]));
              }
              __builtin_amdgcn_sched_barrier(0);   // one row's weights at a time: bounds register pressure
            }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float r = fsum[n][0] + __shfl_xor(fsum[n][0], 32);
          const float g = fsum[n][1] + __shfl_xor(fsum[n][1], 32);
          const float b = fsum[n][2] + __shfl_xor(fsum[n][2], 32);
          if (h == 0) red[w * P + 32 * n + j] = (f32x4){r, g, b, 0.f};
        }
        break;
      }
      // bound of this layer's output per point -> scale of the next operand
      float nscale[NB], iz[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        nscale[n] = x3_scale_for((hdr[16 + l] * Mp[n] + hdr[32 + l]) * 1.01f);
        iz[n] = 1.0f / zs[n];
        amax[n] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            const int k = (2 * t + p) * NB + n;
            float hv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[e] = __builtin_fmaxf(acc[t][n][8 * p + e] * iz[n], 0.f);
            float m = amax[n];
#pragma unroll
            for (int e = 0; e < 8; e += 2) m = __builtin_fmaxf(m, __builtin_fmaxf(hv[e], hv[e + 1]));
            amax[n] = m;
            u32x4 p0, p1;
            split8_f16(hv, p0, p1, nscale[n]);
            own[(k * kAP + 0) * 64] = p0; own[(k * kAP + 1) * 64] = p1;
            __builtin_amdgcn_sched_barrier(0);     // one group at a time: bounds register pressure
          }
#pragma unroll
      for (int n = 0; n < NB; ++n) bscale[n] = nscale[n];
      mbuf ^= 1;
      put_amax(mbuf);
      __syncthreads();                                   // the next layer's inputs (and maxima) are complete
      get_max(mbuf, Mp);
    }
    // ---- the three sums over the waves, tanh, (x + 1) / 2 ------------------------------------------
    if (tid == 0) s_next_tile = drawn;
    __syncthreads();
    next_tile = (int64_t)__builtin_amdgcn_readfirstlane(s_next_tile);        // uniform: the tile's addresses stay scalar
    {
      const int64_t slot = tile * P + tid;
      if (tid < P && slot < count) {
        const f32x4 b_head = *reinterpret_cast<const f32x4*>(a.packed + texp_hbias(s));
        f32x4 r = red[tid];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) {
          const f32x4 q = red[ww * P + tid];
          r.x += q.x; r.y += q.y; r.z += q.z;
        }
        a.rgb[slot * 3] = (tanhf(r.x + b_head.x) + 1.0f) / 2.0f;
        a.rgb[slot * 3 + 1] = (tanhf(r.y + b_head.y) + 1.0f) / 2.0f;
        a.rgb[slot * 3 + 2] = (tanhf(r.z + b_head.z) + 1.0f) / 2.0f;
      }
    }
    __syncthreads();
  }
}

template <int H>
void launch_texture(const TexArgs& a, hipStream_t st) {
  using S = TexTile<H>;
  iso_launch_lds<k_texture_x16<H>>(iso_capped_grid(a.n, S::P, kIdrBlocks), 512, S::kLds, st, a);
}

}  // namespace

extern "C" int iso_texture_form(int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  return tex_form(hidden, n_layers, c_dim, geom, n_freq);
}

extern "C" int64_t iso_texture_raw_floats(int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  if (tex_form(hidden, n_layers, c_dim, geom, n_freq) < 0) return 0;
  const TexShape s = tex_shape(hidden, n_layers, c_dim, geom, n_freq);
  return tex_raw_off(s, n_layers + 1);
}

extern "C" int64_t iso_texture_packed_floats(int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  if (tex_form(hidden, n_layers, c_dim, geom, n_freq) < 0) return 0;
  return texp_end(tex_shape(hidden, n_layers, c_dim, geom, n_freq));
}

extern "C" int iso_texture_pack_weights(const float* raw, float* packed, int hidden, int n_layers, int c_dim, int geom,
                                        int n_freq, void* stream) {
  ISO_REQUIRE(tex_form(hidden, n_layers, c_dim, geom, n_freq) >= 0, ISO_ERR_UNSUPPORTED,
              "iso_texture_pack_weights: unsupported shape (hidden 256/512, 1..8 layers, c_dim <= 256, geom 3/6, n_freq -1..6)");
  ISO_REQUIRE(raw && packed, ISO_ERR_INVALID, "iso_texture_pack_weights: null pointer");
  const TexShape s = tex_shape(hidden, n_layers, c_dim, geom, n_freq);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_texture_stats, dim3(n_layers), dim3(256), 0, st, raw, packed, s);
  hipLaunchKernelGGL(k_texture_pack, dim3(iso_stream_grid(texp_end(s), 256)), dim3(256), 0, st, raw, packed, s);
  ISO_CHECK_LAUNCH("iso_texture_pack_weights");
  return ISO_OK;
}

// [tile counter, 64 B]
extern "C" int64_t iso_texture_workspace_bytes(int64_t n, int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  (void)n; (void)hidden; (void)n_layers; (void)c_dim; (void)geom; (void)n_freq;
  return 64;
}

extern "C" int iso_texture_rgb(const float* points, const float* normals, const float* codes, const float* view_origins,
                               const int32_t* origin_of, int64_t n_origins, float* rgb_out, int64_t n, const float* packed,
                               int hidden, int n_layers, int c_dim, int geom, int n_freq, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  const int form = tex_form(hidden, n_layers, c_dim, geom, n_freq);
  ISO_REQUIRE(form >= 0, ISO_ERR_UNSUPPORTED,
              "iso_texture_rgb: unsupported shape (hidden 256/512, 1..8 layers, c_dim <= 256, geom 3/6, n_freq -1..6)");
  ISO_REQUIRE(n >= 0, ISO_ERR_INVALID, "iso_texture_rgb: negative n");
  if (n == 0) return ISO_OK;
  ISO_REQUIRE(points && rgb_out && packed && workspace, ISO_ERR_INVALID, "iso_texture_rgb: null pointer");
  ISO_REQUIRE((geom == 6) == (normals != nullptr), ISO_ERR_INVALID, "iso_texture_rgb: normals are required iff geom == 6");
  ISO_REQUIRE((c_dim > 0) == (codes != nullptr), ISO_ERR_INVALID, "iso_texture_rgb: codes are required iff c_dim > 0");
  ISO_REQUIRE((n_freq >= 0) == (view_origins != nullptr), ISO_ERR_INVALID,
              "iso_texture_rgb: view_origins are required iff n_freq >= 0");
  ISO_REQUIRE(n_freq < 0 || n_origins >= 1, ISO_ERR_INVALID, "iso_texture_rgb: n_origins must be at least 1");
  ISO_REQUIRE(n_freq >= 0 || !origin_of, ISO_ERR_INVALID, "iso_texture_rgb: origin_of without a view direction");
  ISO_REQUIRE(workspace_bytes >= iso_texture_workspace_bytes(n, hidden, n_layers, c_dim, geom, n_freq), ISO_ERR_INVALID,
              "iso_texture_rgb: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  TexArgs a;
  a.points = points; a.normals = normals; a.codes = codes; a.origins = view_origins; a.origin_of = origin_of;
  a.n_origins = n_origins; a.rgb = rgb_out; a.n = n; a.packed = packed;
  a.s = tex_shape(hidden, n_layers, c_dim, geom, n_freq);
  a.tile_ctr = (int32_t*)workspace;
  iso_zero_words(workspace, 1, st);
  if (form == 616) launch_texture<256>(a, st);
  else launch_texture<512>(a, st);
  ISO_CHECK_LAUNCH("iso_texture_rgb");
  return ISO_OK;
}
