// Shared between texture.hip (the fused forward) and texgrad.hip (the backward): the accepted shapes, the row layout and
// the raw weight layout of the texture network.
#pragma once
#include "iso_common.h"

namespace {

constexpr int kTexMaxL = 8;
constexpr int kTexMaxC = 256;
constexpr int kTexMaxF = 6;
constexpr int kTexK0Max = 320;       // D0 <= 301 padded to a multiple of 64

struct TexShape {
  int H, n_layers, C, G, F;          // F < 0: no view direction
  int V, D0, K0;                     // view slots, row length, padded K of layer 0
};

// The ONE predicate of iso_texture_form / iso_texgrad_form, the size helpers, the packing and the launches.
inline bool tex_shape_ok(int H, int n_layers, int C, int G, int F) {
  return (H == 256 || H == 512) && n_layers >= 1 && n_layers <= kTexMaxL && C >= 0 && C <= kTexMaxC && (G == 3 || G == 6) &&
         F >= -1 && F <= kTexMaxF;
}

inline TexShape tex_shape(int H, int n_layers, int C, int G, int F) {
  TexShape s;
  s.H = H; s.n_layers = n_layers; s.C = C; s.G = G; s.F = F;
  s.V = F < 0 ? 0 : 3 + 6 * F;
  s.D0 = C + G + s.V;
  s.K0 = (s.D0 + 63) / 64 * 64;
  return s;
}

// The refusals iso_texture_rgb and iso_texgrad_backward share, in `fn`'s name.  tex_check_shape comes first; the caller
// answers n == 0 itself, calls tex_check_inputs with `required` = all of its own must-have pointers are there, and goes on
// with the checks of its own.
inline int tex_check_shape(const char* fn, int64_t n, int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  ISO_REQUIRE(tex_shape_ok(hidden, n_layers, c_dim, geom, n_freq), ISO_ERR_UNSUPPORTED,
              "%s: unsupported shape (hidden 256/512, 1..8 layers, c_dim <= 256, geom 3/6, n_freq -1..6)", fn);
  ISO_REQUIRE(n >= 0, ISO_ERR_INVALID, "%s: negative n", fn);
  return ISO_OK;
}

inline int tex_check_inputs(const char* fn, bool required, const float* normals, const float* codes, const float* view_origins,
                            const int32_t* origin_of, int64_t n_origins, int c_dim, int geom, int n_freq) {
  ISO_REQUIRE(required, ISO_ERR_INVALID, "%s: null pointer", fn);
  ISO_REQUIRE((geom == 6) == (normals != nullptr), ISO_ERR_INVALID, "%s: normals are required iff geom == 6", fn);
  ISO_REQUIRE((c_dim > 0) == (codes != nullptr), ISO_ERR_INVALID, "%s: codes are required iff c_dim > 0", fn);
  ISO_REQUIRE((n_freq >= 0) == (view_origins != nullptr), ISO_ERR_INVALID, "%s: view_origins are required iff n_freq >= 0", fn);
  ISO_REQUIRE(n_freq < 0 || n_origins >= 1, ISO_ERR_INVALID, "%s: n_origins must be at least 1", fn);
  ISO_REQUIRE(n_freq >= 0 || !origin_of, ISO_ERR_INVALID, "%s: origin_of without a view direction", fn);
  return ISO_OK;
}

// raw (floats): for l = 0..n_layers: W_l row-major [out][in], b_l[out]; in_0 = D0, out_l = H, head H -> 3
__host__ __device__ inline int tex_in_dim(const TexShape& s, int l) { return l == 0 ? s.D0 : s.H; }
__host__ __device__ inline int tex_out_dim(const TexShape& s, int l) { return l == s.n_layers ? 3 : s.H; }
__host__ __device__ inline int64_t tex_raw_off(const TexShape& s, int l) {
  int64_t o = 0;
  for (int k = 0; k < l; ++k) o += (int64_t)tex_out_dim(s, k) * tex_in_dim(s, k) + tex_out_dim(s, k);
  return o;
}

}  // namespace
