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
// The kernel's body is texture_tile.h (the backward of texgrad.hip recomputes this forward from the same code); here are the
// packing of the weight image and the C entry points.
//   c     = codes[i]                                              (n, C)
//   x     = [c, normal_i, p_i, e(normalize(p_i - origin[origin_of[i]]))]
//   h_0   = relu(W_0 x + b_0),  h_l = relu(W_l h_{l-1} + b_l),  rgb = (tanh(W_n h_{n-1} + b_n) + 1) / 2
#include "idr_common.h"
#include "mfma_split.h"
#include "texture_common.h"
#include "texture_tile.h"

namespace {

// kernel code: 600 + hidden / 16 = k_texture_x16<hidden>; -1: refused (tex_shape_ok of texture_common.h)
int tex_form(int H, int n_layers, int C, int G, int F) { return tex_shape_ok(H, n_layers, C, G, F) ? 600 + H / 16 : -1; }

// per layer: 2^s_l with max |2^s_l W_l| in [512, 1024), the largest row sum of |W_l| and the largest |b_l|
__global__ void k_texture_stats(const float* __restrict__ raw, float* __restrict__ packed, TexShape s) {
  __shared__ float s_m[256];
  const int H = s.H, l = blockIdx.x;
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
  mx = iso_block_max256(mx, s_m); rs = iso_block_max256(rs, s_m); bm = iso_block_max256(bm, s_m);
  if (threadIdx.x == 0) { packed[l] = x3_weight_scale(mx); packed[16 + l] = rs; packed[32 + l] = bm; }
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
      reinterpret_cast<unsigned*>(packed)[o] = tex_f16_word(v, part);
    }
  }
}

// assemble the rows, the layers, the head: tex_forward_tiles of texture_tile.h
template <int H>
__global__ __launch_bounds__(512, 1) void k_texture_x16(TexArgs a) {
  tex_forward_tiles<H, false>(a);
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
  const char* fn = "iso_texture_rgb";
  if (int rc = tex_check_shape(fn, n, hidden, n_layers, c_dim, geom, n_freq)) return rc;
  if (n == 0) return ISO_OK;
  if (int rc = tex_check_inputs(fn, points && rgb_out && packed && workspace, normals, codes, view_origins, origin_of, n_origins,
                                c_dim, geom, n_freq))
    return rc;
  ISO_REQUIRE(workspace_bytes >= iso_texture_workspace_bytes(n, hidden, n_layers, c_dim, geom, n_freq), ISO_ERR_INVALID,
              "iso_texture_rgb: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  TexArgs a;
  a.points = points; a.normals = normals; a.codes = codes; a.origins = view_origins; a.origin_of = origin_of;
  a.n_origins = n_origins; a.rgb = rgb_out; a.n = n; a.packed = packed;
  a.s = tex_shape(hidden, n_layers, c_dim, geom, n_freq);
  a.tile_ctr = (int32_t*)workspace;
  iso_zero_words(workspace, 1, st);
  if (hidden == 256) launch_texture<256>(a, st);
  else launch_texture<512>(a, st);
  ISO_CHECK_LAUNCH("iso_texture_rgb");
  return ISO_OK;
}
