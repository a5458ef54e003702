// Fused SIREN SDF path, gfx950: the C ABI (include/isopoints.h), the ONE decision which step kernel a call takes
// (siren_form), the workspace carve and the iteration set-up of the Newton projection, sphere tracing and the plain
// evaluation (siren_run on sdf_driver.h).  The step kernels are in siren_f32.hip (f32 MFMA) and siren_x3.hip (split fp16).
//
// Reference semantics: Siren.forward (DSS/models/common.py:140-165, SineLayer :86-87) evaluated with autograd.grad inside
// UniformProjection._compute_sdf_and_grad (levelset_sampling.py:142-170) and iterated by _project_points (:313-342).
// Newton: one launch = one evaluation (+ move) over the list of still active points; survivors are appended to the next
// list with a wave aggregated atomic, so converged points cost nothing in later launches (the reference's boolean-mask
// compaction, without host syncs).
#include <stdlib.h>
#include <string.h>
#include "siren_common.h"
#include "sdf_driver.h"

namespace {

bool siren_shape_ok(int H, int L) {
  return (H == 64 || H == 128 || H == 256) && L >= 0 && L <= 8;
}

// 0 = f32 MFMA kernel (siren_f32.hip), 1 = split-fp16 MFMA kernels (siren_x3.hip) where they apply.
// Default 1; the environment variable ISO_SIREN_GEMM=f32 selects 0 at load time.
int g_gemm_mode = -1;
int gemm_mode() {
  if (g_gemm_mode < 0) {
    const char* e = getenv("ISO_SIREN_GEMM");
    g_gemm_mode = (e && (!strcmp(e, "f32") || !strcmp(e, "0"))) ? 0 : 1;
  }
  return g_gemm_mode;
}

// Form of the split-fp16 gradient step at hidden size 256 (iso_siren_set_step_form): 0 = eight waves per workgroup, the
// derivative stash in global memory; 1 (the default) = four waves of 512 registers, the stash in LDS and registers, for
// two and three hidden layers of an uncoded network.  Results do not depend on it.
int g_step_form = 1;

// The ONE place that decides which kernel a call takes (iso_siren_step_kernel reports it, siren_launch_form launches it,
// the Newton tail and the tile counters follow it).  value_only: tracing, or an evaluation without grad_out.
//   100 + H/16  k_siren_step<H/16, coded>                          f32 mode; or H = 64; or no hidden layer
//   200 + H/16  k_siren_step_x3<H, ., ., ., true, coded>           split fp16, value only
//   308         k_siren_step_x3<128, 4, 3, 1, false, coded>        split fp16, gradient, H = 128
//   416         k_siren_step_x3_both<256, 8, 3, 1, coded>          split fp16, gradient, H = 256, unless 516
//   516         k_siren_step_x3_both_oc<256, 3, 1, false, L>       step form 1, uncoded, L = 2 / 3
//   -1          a shape siren_shape_ok refuses
int siren_form(int hidden, int n_hidden, bool value_only, bool coded) {
  if (!siren_shape_ok(hidden, n_hidden)) return -1;
  const int NT = hidden / 16;
  if (gemm_mode() == 0 || !siren_x3_supported(hidden, n_hidden)) return 100 + NT;
  if (value_only) return 200 + NT;
  if (hidden == 256 && g_step_form == 1 && (n_hidden == 2 || n_hidden == 3) && !coded) return 500 + NT;
  return (hidden == 128 ? 300 : 400) + NT;
}

int siren_launch_form(int form, const SirenCodedArgs& a, int64_t n, hipStream_t s) {
  switch (form / 100) {
    case 1: return siren_f32_launch(a, 16 * (form % 100), n, s);
    case 2: case 3: case 4: case 5: return siren_x3_launch(form, a, n, s);
    default: return -1;
  }
}

// 4xx / 5xx: one launch serves a list cut at siren_split_point into 96-point and 32-point tiles, drawn from two counters
// (SirenArgs::tile_ctr), and the late Newton iterations are one tail launch
bool form_splits(int form) { return form / 100 >= 4; }

// From which iteration on the Newton projection runs as ONE tail launch (k_siren_tail_x3): the lists of the first
// iterations are long (launch-per-iteration, 96-point tiles), the late ones a few hundred points or none.  T >= 6: after
// four launches; shorter projections (the T = 3 re-projection of resample): after two.  iso_siren_set_tail_from
// overrides (0: never, the launch-per-iteration form).  max_iters + 1: no tail.
int g_tail_from = -1;       // -1: default policy, 0: never, k > 0: from iteration k
int siren_tail_first(int form, int max_iters) {
  if (!form_splits(form) || g_tail_from == 0) return max_iters + 1;
  if (g_tail_from > 0) return g_tail_from;
  return max_iters >= 6 ? 4 : 2;
}

int g_dyn_tiles = -1;       // -1: the default (on), 0 / 1: iso_siren_set_drawn_tiles (off: static tile assignment, tests)

int64_t stash_floats_any(int H, int L) {
  int64_t a = siren_f32_stash_floats(H, L);
  int64_t b = siren_x3_supported(H, L) ? siren_x3_stash_floats(H, L) : 0;
  return a > b ? a : b;
}

// The workspace, as byte offsets: [stash floats][idx A n][idx B n][tail lists][tail counters][counts 64][tile counters:
// two per launch].  Tail lists: private survivor lists of the tail launch's workgroups, two of tail_cap entries each (a
// workgroup's share of a list is at most ceil(tiles / blocks) tiles of 32), then their two counters each.
constexpr int kTileCtrInts = 128;     // (max_iters <= 60: 61 launches)
struct SirenCarve {
  int64_t idxA, idxB, tail, tail_counts, counts, tile_ctr, end, tail_cap;
};
SirenCarve siren_carve(int64_t n, int H, int L) {
  if (n < 0) n = 0;
  const int64_t blocks = siren_x3_tail_blocks(), tiles = (n + 31) / 32;
  SirenCarve c;
  c.tail_cap = ((tiles + blocks - 1) / blocks + 1) * 32;
  c.idxA = stash_floats_any(H, L) * 4;
  c.idxB = c.idxA + n * 4;
  c.tail = c.idxB + n * 4;
  c.tail_counts = c.tail + blocks * 2 * c.tail_cap * 4;
  c.counts = c.tail_counts + blocks * 2 * 4;        // counts[it] = size of the list consumed by launch `it`
  c.tile_ctr = c.counts + 64 * 4;                   // [launch][2], zeroed with the counts
  c.end = c.tile_ctr + kTileCtrInts * 4 + 64;
  return c;
}

__global__ void k_siren_zero(int32_t* c, int n, int32_t* tc, int m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) c[i] = 0;
  if (i < m) tc[i] = 0;
}

// code_bias / code_of as SirenCodedArgs documents them; null code_bias: the uncoded network (the image's own b0)
struct SirenCodes { const float* bias; const int32_t* of; };

int siren_codes_ok(const char* who, const float* code_bias, const int32_t* code_of, int64_t n_codes) {
  ISO_REQUIRE(code_bias && n_codes >= 1 && (code_of || n_codes == 1), ISO_ERR_INVALID,
              "%s: needs a bias table of n_codes >= 1 rows (and code_of when n_codes > 1)", who);
  return ISO_OK;
}

// The one body of iso_project_siren, iso_trace_siren (c.dirs) and iso_siren_sdf_grad (c.eval_only), coded or not.
// ptrs_ok: the entry's own pointers are there.  Around a launch of the shared schedule (sdf_driver.h): the pair of tile
// counters of a split form, and from siren_tail_first on ONE tail launch for all the iterations left.
int siren_run(const SdfCall& c, bool ptrs_ok, const float* packed, int hidden, int n_hidden, float omega_first,
              float omega_hidden, void* workspace, int64_t workspace_bytes, void* stream, SirenCodes codes) {
  ISO_REQUIRE(siren_shape_ok(hidden, n_hidden), ISO_ERR_UNSUPPORTED,
              "%s: hidden must be 64/128/256 and 0<=n_hidden<=8 (got %d, %d)", c.who, hidden, n_hidden);
  if (const int rc = sdf_call_check(c, ptrs_ok && packed && workspace)) return rc < 0 ? rc : ISO_OK;
  const SirenCarve cv = siren_carve(c.n, hidden, n_hidden);
  // (an evaluation needs the stash alone; a workspace of the projection's size -- what the Python side allocates -- has
  // room for its two tile counters too)
  ISO_REQUIRE(workspace_bytes >= (c.eval_only ? cv.idxA : cv.end), ISO_ERR_WORKSPACE, "%s: workspace too small", c.who);
  hipStream_t s = (hipStream_t)stream;
  auto at = [&](int64_t off) { return (int32_t*)((char*)workspace + off); };
  const int form = siren_form(hidden, n_hidden, c.value_only(), codes.bias != nullptr);
  static_assert(2 * (kSdfMaxIters + 1) <= kTileCtrInts, "two tile counters per launch");
  const bool dyn_tiles = form_splits(form) && g_dyn_tiles != 0 && workspace_bytes >= cv.end;
  const int tail_from = siren_tail_first(form, c.max_iters);
  if (c.eval_only) {
    if (dyn_tiles) hipLaunchKernelGGL(k_siren_zero, dim3(1), dim3(64), 0, s, at(cv.tile_ctr), 2, nullptr, 0);
  } else {
    const int blocks = siren_x3_tail_blocks();
    hipLaunchKernelGGL(k_siren_zero, dim3((2 * blocks + 255) / 256), dim3(256), 0, s, at(cv.counts), 64 + kTileCtrInts,
                       at(cv.tail_counts), tail_from <= c.max_iters ? 2 * blocks : 0);
  }
  SirenCodedArgs a;
  a.packed = packed; a.stash = (float*)workspace; a.L = n_hidden;
  a.w0 = omega_first; a.wh = omega_hidden;
  a.code_bias = codes.bias; a.code_of = codes.of;
  return sdf_run(c, a, SdfLists{at(cv.idxA), at(cv.idxB), at(cv.counts)}, s, [&](SirenCodedArgs& x, int it) {
    x.tile_ctr = dyn_tiles ? at(cv.tile_ctr) + 2 * it : nullptr;
    if (it >= tail_from && it > 0) {        // iterations it .. max_iters in one launch
      x.tail_lists = at(cv.tail); x.tail_counts = at(cv.tail_counts); x.iter_counts = at(cv.counts); x.tail_cap = (int)cv.tail_cap;
      x.it_first = it; x.it_last = c.max_iters;
      ISO_REQUIRE(siren_x3_launch_tail(x, hidden, s) == 0, ISO_ERR_UNSUPPORTED, "%s: no tail kernel for hidden size %d", c.who, hidden);
      return kSdfStop;
    }
    ISO_REQUIRE(siren_launch_form(form, x, c.n, s) == 0, ISO_ERR_UNSUPPORTED, "%s: unsupported hidden size %d", c.who, hidden);
    return ISO_OK;
  });
}

}  // namespace

extern "C" int64_t iso_siren_raw_floats(int hidden, int n_hidden) {
  int64_t H = hidden;
  return H * 3 + H + (int64_t)n_hidden * (H * H + H) + H + 1;
}

extern "C" int64_t iso_siren_packed_floats(int hidden, int n_hidden) {
  return siren_packed_total(hidden, n_hidden);
}

extern "C" int iso_siren_set_gemm_mode(int mode) {
  ISO_REQUIRE(mode == 0 || mode == 1, ISO_ERR_INVALID, "iso_siren_set_gemm_mode: mode must be 0 (f32 MFMA) or 1 (split fp16)");
  g_gemm_mode = mode;
  return ISO_OK;
}
extern "C" int iso_siren_get_gemm_mode(void) { return gemm_mode(); }

extern "C" int iso_siren_set_step_form(int form) {
  ISO_REQUIRE(form == 0 || form == 1, ISO_ERR_INVALID, "iso_siren_set_step_form: 0 (eight waves, global stash) or 1 (four waves, stash on chip)");
  g_step_form = form;
  return ISO_OK;
}
extern "C" int iso_siren_get_step_form(void) { return g_step_form; }

extern "C" int iso_siren_set_drawn_tiles(int on) {
  ISO_REQUIRE(on >= -1 && on <= 1, ISO_ERR_INVALID, "iso_siren_set_drawn_tiles: -1 (default), 0 or 1");
  g_dyn_tiles = on;
  return ISO_OK;
}

extern "C" int iso_siren_set_tail_from(int first_tail_iteration) {
  ISO_REQUIRE(first_tail_iteration >= -1, ISO_ERR_INVALID, "iso_siren_set_tail_from: -1 (default), 0 (never) or an iteration >= 1");
  g_tail_from = first_tail_iteration;
  return ISO_OK;
}

extern "C" int iso_siren_step_kernel(int hidden, int n_hidden, int value_only, int coded) {
  return siren_form(hidden, n_hidden, value_only != 0, coded != 0);
}
// the form that serves a gradient step of this shape as things are set now (0 also where the split-fp16 kernels do not run)
extern "C" int iso_siren_step_form_used(int hidden, int n_hidden, int coded) {
  return siren_form(hidden, n_hidden, false, coded != 0) / 100 == 5 ? 1 : 0;
}
extern "C" int iso_siren_step_launches(int hidden, int n_hidden, int max_iters) {
  if (max_iters < 0) return 0;
  const int from = siren_tail_first(siren_form(hidden, n_hidden, false, false), max_iters);
  return from <= max_iters && from > 0 ? from + 1 : max_iters + 1;
}

extern "C" int iso_siren_pack_weights(const float* raw, float* packed, int hidden,
                                      int n_hidden, void* stream) {
  ISO_REQUIRE(siren_shape_ok(hidden, n_hidden), ISO_ERR_UNSUPPORTED,
              "iso_siren_pack_weights: hidden must be 64/128/256 and 0<=n_hidden<=8 (got %d, %d)",
              hidden, n_hidden);
  ISO_REQUIRE(raw && packed, ISO_ERR_INVALID, "iso_siren_pack_weights: null pointer");
  siren_f32_pack(raw, packed, hidden, n_hidden, (hipStream_t)stream);
  if (hidden % 32 == 0) siren_x3_pack(raw, packed, hidden, n_hidden, (hipStream_t)stream);
  ISO_CHECK_LAUNCH("iso_siren_pack_weights");
  return ISO_OK;
}

extern "C" int64_t iso_project_siren_workspace_bytes(int64_t n, int hidden, int n_hidden) {
  return siren_carve(n, hidden, n_hidden).end;
}
extern "C" int64_t iso_project_siren_counts_offset(int64_t n, int hidden, int n_hidden) {
  return siren_carve(n, hidden, n_hidden).counts;
}

// ---- latent-conditioned SIREN: the per-code bias table of layer 0 ------------------------------
// The reference concatenates the code in front of the point (DSS/models/common.py:150-152), so layer 0 of code u is
// sin(w0 (W0[:, C:] x + b_u)) with b_u = b0 + W0[:, :C] c_u: the code only moves layer 0's bias.
// table[u * Hp + f] = b0[f] + sum_k W0c[f][k] c_u[k], accumulated in double in ONE fixed order (b0, then k = 0, 1, .. by
// fma; products of two floats are exact in double) and rounded once to f32; the padded features f >= H get 0.
__global__ void k_siren_fold_codes(const float* __restrict__ w0c, const float* __restrict__ b0,
                                   const float* __restrict__ codes, float* __restrict__ table, int H, int Hp, int C,
                                   int64_t U) {
  const int64_t total = U * Hp;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = o / Hp;
    const int f = (int)(o - u * Hp);
    float v = 0.f;
    if (f < H) {
      double acc = (double)b0[f];
      const float* wr = w0c + (int64_t)f * C;
      const float* cu = codes + u * C;
      for (int k = 0; k < C; ++k) acc = fma((double)wr[k], (double)cu[k], acc);
      v = (float)acc;
    }
    table[o] = v;
  }
}

extern "C" int iso_siren_fold_codes(const float* w0c, const float* b0, const float* codes, float* table, int hidden,
                                    int padded_hidden, int c_dim, int64_t n_codes, void* stream) {
  ISO_REQUIRE(hidden >= 1 && padded_hidden >= hidden && c_dim >= 1 && n_codes >= 0, ISO_ERR_INVALID,
              "iso_siren_fold_codes: bad sizes (hidden %d, padded %d, c_dim %d, codes %lld)", hidden, padded_hidden,
              c_dim, (long long)n_codes);
  if (n_codes == 0) return ISO_OK;
  ISO_REQUIRE(w0c && b0 && codes && table, ISO_ERR_INVALID, "iso_siren_fold_codes: null pointer");
  const int64_t total = n_codes * padded_hidden;
  hipLaunchKernelGGL(k_siren_fold_codes, dim3(iso_stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, w0c, b0,
                     codes, table, hidden, padded_hidden, c_dim, n_codes);
  ISO_CHECK_LAUNCH("iso_siren_fold_codes");
  return ISO_OK;
}

// ---- the three entries, uncoded and coded: siren_run with the entry's own pointers checked ------
static int project_siren(const char* who, const float* pts_in, float* pts_out, float* normals_out, uint8_t* mask_out,
                         int64_t n, const float* packed, int hidden, int n_hidden, float omega_first, float omega_hidden,
                         int max_iters, float tol, void* workspace, int64_t workspace_bytes, void* stream, SirenCodes codes) {
  const SdfCall c = {who, pts_in, pts_out, normals_out, mask_out, nullptr, nullptr, n, max_iters, tol, false};
  return siren_run(c, pts_in && pts_out && normals_out && mask_out, packed, hidden, n_hidden, omega_first, omega_hidden,
                   workspace, workspace_bytes, stream, codes);
}

extern "C" int iso_project_siren(const float* pts_in, float* pts_out, float* normals_out,
                                 uint8_t* mask_out, int64_t n, const float* packed,
                                 int hidden, int n_hidden, float omega_first,
                                 float omega_hidden, int max_iters, float tol,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return project_siren("iso_project_siren", pts_in, pts_out, normals_out, mask_out, n, packed, hidden, n_hidden, omega_first,
                       omega_hidden, max_iters, tol, workspace, workspace_bytes, stream, SirenCodes{nullptr, nullptr});
}

extern "C" int iso_project_siren_coded(const float* pts_in, float* pts_out, float* normals_out,
                                       uint8_t* mask_out, int64_t n, const float* packed,
                                       int hidden, int n_hidden, float omega_first,
                                       float omega_hidden, int max_iters, float tol,
                                       void* workspace, int64_t workspace_bytes, void* stream,
                                       const float* code_bias, const int32_t* code_of, int64_t n_codes) {
  const char* who = "iso_project_siren_coded";
  if (int rc = siren_codes_ok(who, code_bias, code_of, n_codes)) return rc;
  return project_siren(who, pts_in, pts_out, normals_out, mask_out, n, packed, hidden, n_hidden, omega_first, omega_hidden,
                       max_iters, tol, workspace, workspace_bytes, stream, SirenCodes{code_bias, code_of});
}

static int trace_siren(const char* who, const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                       uint8_t* mask_out, int64_t n, const float* packed, int hidden, int n_hidden, float omega_first,
                       float omega_hidden, float alpha, float bound, int max_iters, float tol, void* workspace,
                       int64_t workspace_bytes, void* stream, SirenCodes codes) {
  const SdfCall c = {who, ray0, pts_out, nullptr, mask_out, sdf_out, nullptr, n, max_iters, tol, false, dirs, alpha, bound};
  return siren_run(c, ray0 && dirs && pts_out && sdf_out && mask_out, packed, hidden, n_hidden, omega_first, omega_hidden,
                   workspace, workspace_bytes, stream, codes);
}

extern "C" int iso_trace_siren(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                               uint8_t* mask_out, int64_t n, const float* packed, int hidden,
                               int n_hidden, float omega_first, float omega_hidden, float alpha,
                               float bound, int max_iters, float tol, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  return trace_siren("iso_trace_siren", ray0, dirs, pts_out, sdf_out, mask_out, n, packed, hidden, n_hidden, omega_first,
                     omega_hidden, alpha, bound, max_iters, tol, workspace, workspace_bytes, stream, SirenCodes{nullptr, nullptr});
}

extern "C" int iso_trace_siren_coded(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                                     uint8_t* mask_out, int64_t n, const float* packed, int hidden,
                                     int n_hidden, float omega_first, float omega_hidden, float alpha,
                                     float bound, int max_iters, float tol, void* workspace,
                                     int64_t workspace_bytes, void* stream,
                                     const float* code_bias, const int32_t* code_of, int64_t n_codes) {
  const char* who = "iso_trace_siren_coded";
  if (int rc = siren_codes_ok(who, code_bias, code_of, n_codes)) return rc;
  return trace_siren(who, ray0, dirs, pts_out, sdf_out, mask_out, n, packed, hidden, n_hidden, omega_first, omega_hidden,
                     alpha, bound, max_iters, tol, workspace, workspace_bytes, stream, SirenCodes{code_bias, code_of});
}

static int sdf_grad_siren(const char* who, const float* pts, float* sdf_out, float* grad_out, int64_t n,
                          const float* packed, int hidden, int n_hidden, float omega_first, float omega_hidden,
                          void* workspace, int64_t workspace_bytes, void* stream, SirenCodes codes) {
  const SdfCall c = {who, pts, nullptr, nullptr, nullptr, sdf_out, grad_out, n, 0, 0.f, true};
  return siren_run(c, pts && sdf_out, packed, hidden, n_hidden, omega_first, omega_hidden, workspace, workspace_bytes, stream,
                   codes);
}

extern "C" int iso_siren_sdf_grad(const float* pts, float* sdf_out, float* grad_out,
                                  int64_t n, const float* packed, int hidden,
                                  int n_hidden, float omega_first, float omega_hidden,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return sdf_grad_siren("iso_siren_sdf_grad", pts, sdf_out, grad_out, n, packed, hidden, n_hidden, omega_first, omega_hidden,
                        workspace, workspace_bytes, stream, SirenCodes{nullptr, nullptr});
}

extern "C" int iso_siren_sdf_grad_coded(const float* pts, float* sdf_out, float* grad_out,
                                        int64_t n, const float* packed, int hidden,
                                        int n_hidden, float omega_first, float omega_hidden,
                                        void* workspace, int64_t workspace_bytes, void* stream,
                                        const float* code_bias, const int32_t* code_of, int64_t n_codes) {
  const char* who = "iso_siren_sdf_grad_coded";
  if (int rc = siren_codes_ok(who, code_bias, code_of, n_codes)) return rc;
  return sdf_grad_siren(who, pts, sdf_out, grad_out, n, packed, hidden, n_hidden, omega_first, omega_hidden, workspace,
                        workspace_bytes, stream, SirenCodes{code_bias, code_of});
}
