// Fused IDR-style SDF path, gfx950: the C ABI (include/isopoints.h), the ONE decision which step kernel a call takes
// (idr_form), the workspace carve and the iteration set-up of the Newton projection, sphere tracing and the plain
// evaluation (idr_run on sdf_driver.h).  The step kernels are in idr_f32.hip (f32 MFMA) and idr_x16.hip (split fp16).
//
// Reference network: SDF.forward, DSS/models/common.py:220-310 (based on IDR / SAL):
//   e(x)   = [x, sin(2^k x), cos(2^k x)]_{k<F}                       (get_embedder :205-217)
//   h_0    = softplus_b(W_0 e + b_0)
//   h_l    = softplus_b(W_l in_l + b_l),  in_l = [h_{l-1}, e]/sqrt(2) when l == skip  (:297-298)
//   sdf    = tanh(W_n h_{n-1} + b_n)                                  (:305)
// with weight-normalised linears (:277-278; the effective weights g*v/|v| are formed by the
// caller), beta = 100, torch's softplus threshold 20.  Layer skip-1 outputs H - D0 features so
// that the concatenation is H wide (:251-252).
#include <stdlib.h>
#include "idr_common.h"
#include "sdf_driver.h"

namespace {

// 1 = split-fp16 kernel (idr_x16.hip) where idr_x16_supported: H = 256 / 512 with encodings of <= 39 slots; 0 = the f32-MFMA
// kernels of idr_f32.hip for every shape.  Default 1; ISO_IDR_GEMM=f32 in the environment selects 0 at load time.
int g_idr_gemm_mode = -1;
int idr_gemm_mode() {
  if (g_idr_gemm_mode < 0) {
    const char* e = getenv("ISO_IDR_GEMM");
    g_idr_gemm_mode = (e && e[0] == 'f') ? 0 : 1;
  }
  return g_idr_gemm_mode;
}

// The ONE place that decides which kernel a call takes (iso_idr_step_form reports it, idr_launch_form launches it):
//   100 + NT  k_idr_step<NT>            200 + NT  k_idr_step_fs<NT, false>      300 + NT  k_idr_step_fs<NT, true>
//   400 + NT  k_idr_step_x16<16 NT, ., false>                                   500 + NT  k_idr_step_x16<16 NT, ., true>
//   -1        a shape idr_shape_ok refuses
int idr_form(int H, int n_layers, int skip, int F, bool value_only) {
  if (!idr_shape_ok(H, n_layers, skip, F)) return -1;
  const int NT = H / 16, D0 = 3 + 6 * F;
  if (idr_gemm_mode() == 1 && idr_x16_supported(H, n_layers, skip, F)) return (value_only ? 500 : 400) + NT;
  // H = 128 leaves only 32 MFMAs per q-chunk and wave: the staged kernel is 7 % faster there
  // (value-only evaluations always take the feature-split form where it exists: the staged kernel has no forward-only form)
  if ((NT >= 16 || value_only) && D0 <= kIdrFsEncRows) return (value_only ? 300 : 200) + NT;
  return 100 + NT;
}

int idr_launch_form(int form, const IdrArgs& a, int64_t n, hipStream_t st) {
  // (the staged kernel serves both; every other form was chosen for the value_only the arguments must carry)
  const bool value_form = form / 100 == 3 || form / 100 == 5;
  if (form >= 200 && value_form != (a.fwd_only != 0)) return -1;
  switch (form / 100) {
    case 1: case 2: case 3: return idr_f32_launch(form, a, n, st);
    case 4: case 5: return idr_x16_launch(form, a, n, st);
    default: return -1;
  }
}

IdrShape mk_shape(int H, int n_layers, int skip, int F) { return IdrShape{H, n_layers, skip, F, 3 + 6 * F}; }

int64_t idr_stash_floats(int H, int n_layers) {
  const int64_t a = idr_f32_stash_floats(H, n_layers), b = idr_x16_stash_floats(H, n_layers);
  return a > b ? a : b;
}

__global__ void k_idr_zero(int32_t* c, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) c[i] = 0;
}

int g_idr_dyn_tiles = -1;        // -1: the default (on), 0 / 1: iso_idr_set_drawn_tiles (off: every gridDim-th tile, tests)

}  // namespace

extern "C" int64_t iso_idr_raw_floats(int hidden, int n_layers, int skip_layer, int n_freq) {
  IdrShape s = mk_shape(hidden, n_layers, skip_layer, n_freq);
  return idr_raw_off(s, n_layers + 1);
}
extern "C" int iso_idr_set_gemm_mode(int mode) {
  ISO_REQUIRE(mode == 0 || mode == 1, ISO_ERR_INVALID, "iso_idr_set_gemm_mode: mode must be 0 (f32 MFMA) or 1 (split fp16)");
  g_idr_gemm_mode = mode;
  return ISO_OK;
}

extern "C" int iso_idr_get_gemm_mode(void) { return idr_gemm_mode(); }

extern "C" int iso_idr_step_form(int hidden, int n_layers, int skip_layer, int n_freq, int value_only) {
  return idr_form(hidden, n_layers, skip_layer, n_freq, value_only != 0);
}

extern "C" int iso_idr_set_drawn_tiles(int on) {
  ISO_REQUIRE(on >= -1 && on <= 1, ISO_ERR_INVALID, "iso_idr_set_drawn_tiles: -1 (default), 0 or 1");
  g_idr_dyn_tiles = on;
  return ISO_OK;
}

// (the packed buffer always has room for the split-fp16 images: its size depends neither on the environment nor on the mode)
extern "C" int64_t iso_idr_packed_floats(int hidden, int n_layers) {
  return idr_total(hidden, n_layers) + idr_x16_floats(hidden, n_layers);
}

extern "C" int iso_idr_pack_weights(const float* raw, float* packed, int hidden, int n_layers,
                                    int skip_layer, int n_freq, void* stream) {
  ISO_REQUIRE(idr_shape_ok(hidden, n_layers, skip_layer, n_freq), ISO_ERR_UNSUPPORTED,
              "iso_idr_pack_weights: unsupported shape (hidden 128/256/512, 2..12 layers, <=10 frequencies)");
  ISO_REQUIRE(raw && packed, ISO_ERR_INVALID, "iso_idr_pack_weights: null pointer");
  const IdrShape s = mk_shape(hidden, n_layers, skip_layer, n_freq);
  idr_f32_pack(raw, packed, s, (hipStream_t)stream);
  if (idr_x16_supported(hidden, n_layers, skip_layer, n_freq)) idr_x16_pack(raw, packed, s, (hipStream_t)stream);
  ISO_CHECK_LAUNCH("iso_idr_pack_weights");
  return ISO_OK;
}

extern "C" int64_t iso_project_idr_workspace_bytes(int64_t n, int hidden, int n_layers) {
  if (n < 0) n = 0;
  return idr_stash_floats(hidden, n_layers) * 4 + 2 * n * 4 + 128 * 4 + 64;      // [stash][idx A][idx B][counts 64][tile counters 64]
}

// The one body of iso_project_idr, iso_trace_idr (c.dirs) and iso_idr_sdf_grad (c.eval_only); the entry has checked its
// own pointers.  The split-fp16 kernel draws its tiles from one counter per launch, zeroed with the counts.
static int idr_run(const SdfCall& c, const float* packed, IdrShape shape, float beta, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(idr_shape_ok(shape.H, shape.n_layers, shape.skip, shape.F), ISO_ERR_UNSUPPORTED,
              "%s: unsupported shape (hidden 128/256/512, 2..12 layers, <=10 frequencies)", c.who);
  if (const int rc = sdf_call_check(c, packed && workspace)) return rc < 0 ? rc : ISO_OK;
  ISO_REQUIRE(workspace_bytes >= iso_project_idr_workspace_bytes(c.n, shape.H, shape.n_layers), ISO_ERR_WORKSPACE,
              "%s: workspace too small", c.who);
  hipStream_t st = (hipStream_t)stream;
  float* stash = (float*)workspace;
  int32_t* idxA = (int32_t*)(stash + idr_stash_floats(shape.H, shape.n_layers));
  int32_t* counts = idxA + 2 * c.n;
  int32_t* tile_ctr = counts + 64;
  const int form = idr_form(shape.H, shape.n_layers, shape.skip, shape.F, c.value_only());
  const bool dyn_tiles = form >= 400 && g_idr_dyn_tiles != 0;
  if (c.eval_only) {
    if (dyn_tiles) hipLaunchKernelGGL(k_idr_zero, dim3(1), dim3(64), 0, st, tile_ctr, 1);
  } else {
    hipLaunchKernelGGL(k_idr_zero, dim3(2), dim3(64), 0, st, counts, 128);
  }
  IdrArgs a;
  a.packed = packed; a.stash = stash; a.s = shape; a.beta = beta;
  return sdf_run(c, a, SdfLists{idxA, idxA + c.n, counts}, st, [&](IdrArgs& x, int it) {
    x.tile_ctr = dyn_tiles ? tile_ctr + it : nullptr;
    ISO_REQUIRE(idr_launch_form(form, x, c.n, st) == 0, ISO_ERR_UNSUPPORTED, "%s: unsupported hidden size", c.who);
    return ISO_OK;
  });
}

extern "C" int iso_project_idr(const float* pts_in, float* pts_out, float* normals_out,
                               uint8_t* mask_out, int64_t n, const float* packed, int hidden,
                               int n_layers, int skip_layer, int n_freq, float beta, int max_iters,
                               float tol, void* workspace, int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(n == 0 || (pts_in && pts_out && normals_out && mask_out), ISO_ERR_INVALID,
              "iso_project_idr: null pointer");
  const SdfCall c = {"iso_project_idr", pts_in, pts_out, normals_out, mask_out, nullptr, nullptr, n, max_iters, tol, false};
  return idr_run(c, packed, mk_shape(hidden, n_layers, skip_layer, n_freq), beta, workspace, workspace_bytes, stream);
}

extern "C" int iso_idr_sdf_grad(const float* pts, float* sdf_out, float* grad_out, int64_t n,
                                const float* packed, int hidden, int n_layers, int skip_layer,
                                int n_freq, float beta, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  ISO_REQUIRE(n == 0 || (pts && sdf_out), ISO_ERR_INVALID, "iso_idr_sdf_grad: null pointer");
  const SdfCall c = {"iso_idr_sdf_grad", pts, nullptr, nullptr, nullptr, sdf_out, grad_out, n, 0, 0.f, true};
  return idr_run(c, packed, mk_shape(hidden, n_layers, skip_layer, n_freq), beta, workspace, workspace_bytes, stream);
}

extern "C" int iso_trace_idr(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                             uint8_t* mask_out, int64_t n, const float* packed, int hidden,
                             int n_layers, int skip_layer, int n_freq, float beta, float alpha,
                             float bound, int max_iters, float tol, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  ISO_REQUIRE(n == 0 || (ray0 && dirs && pts_out && sdf_out && mask_out), ISO_ERR_INVALID,
              "iso_trace_idr: null pointer");
  const SdfCall c = {"iso_trace_idr", ray0, pts_out, nullptr, mask_out, sdf_out, nullptr, n, max_iters, tol, false,
                     dirs, alpha, bound};
  return idr_run(c, packed, mk_shape(hidden, n_layers, skip_layer, n_freq), beta, workspace, workspace_bytes, stream);
}
