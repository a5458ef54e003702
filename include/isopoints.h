/*
 * isopoints.h -- C ABI of the MI355X (gfx950) iso-point hot path.
 *
 * One shared library (libisopoints_hip.so), plain pointers + sizes, no torch
 * types.  Every pointer is a DEVICE pointer unless its name ends in `_host`.
 * Every entry point enqueues work on `stream` (a hipStream_t passed as void*,
 * NULL = default stream) and returns without synchronising, except where the
 * comment says "syncs".  Return value: ISO_OK (0) or a negative ISO_ERR_*; the
 * message for the last error of the calling thread is iso_last_error().
 * Nothing is allocated inside the library: outputs and workspaces are caller
 * owned (the `*_bytes` helpers size them).  Thread-safe per stream.
 *
 * Each entry point cites the reference interface it stands in for
 * (paths relative to the yifita/iso-points checkout).
 */
#ifndef ISOPOINTS_H_
#define ISOPOINTS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISO_OK 0
#define ISO_ERR_INVALID (-1)     /* bad argument (shape, null pointer, range) */
#define ISO_ERR_UNSUPPORTED (-2) /* valid but outside what the kernels cover   */
#define ISO_ERR_LAUNCH (-3)      /* HIP launch / runtime failure               */
#define ISO_ERR_WORKSPACE (-4)   /* caller workspace too small                 */

const char* iso_version(void);
const char* iso_last_error(void);

/* ------------------------------------------------------------------------
 * A. Newton level-set projection
 *    replaces UniformProjection._project_points + _compute_sdf_and_grad
 *    (DSS/models/levelset_sampling.py:290-351, :142-170).
 *
 *    Per point (points are independent, so the reference's boolean-mask
 *    compaction is an in-register `active` flag here):
 *      repeat: f,g = SDF(p), grad SDF(p); normal = g;
 *              if |f| <= tol -> converged, stop; if it == max_iters -> stop;
 *              m = f*g/sdeno(|g|^2,1e-17); m = m/max(|m|,1e-15)*min(|m|,0.1);
 *              p -= m
 *    points (n,3) f32 packed; normals_out (n,3) = last evaluated gradient (NOT
 *    normalised); mask_out (n) u8 = converged.  In-place (pts_out == pts_in)
 *    is allowed.
 * ---------------------------------------------------------------------- */

/* analytic SDF |x-c| - radius (BASELINE.json configs[0], SURVEY 8(d) cfg 1/3a) */
int iso_project_sphere(const float* pts_in, float* pts_out, float* normals_out,
                       uint8_t* mask_out, int64_t n, float cx, float cy,
                       float cz, float radius, int max_iters, float tol,
                       void* stream);

/* What a projection launch does ON THE SIDE for the stages that consume its result in the iso-point cycle, so that they
 * need no pass of their own over the points it has just written (all pointers device memory):
 *   - the bounding box of the projected points is added to the PENDING BOX of the brick workspace grid_ws (section E;
 *     required, initialised).  iso_bricks_build_pending then makes the grid's header from it -- no box pass, no
 *     launch in between; iso_bricks_box_take returns it as 8 floats (what N ranks all-gather) and clears it.
 *   - views != NULL: the renderable mask of every point (iso_splat_view_mask's rule; normals = the projection's own
 *     normals_out) -> mask_out, and the renderable points per 256-point tile and view -> front_ws
 *     (iso_splat_front_workspace_bytes).  The scan of iso_splat_view_mask_scan (chunk table in front_ws, first_idx_out,
 *     num_pts_out, view_total_out) is done by iso_bricks_build_pending when it is handed the same struct -- the grid
 *     it builds carries the mask as payload, so the two always go together in the cycle.
 * Reference: the consumers are UniformProjection._create_tree (levelset_sampling.py:110-140: bbox of the cloud),
 * SurfaceSplatting._filter_points_with_invalid_depth / backface culling (rasterizer.py:184-254).          */
typedef struct iso_follow {
  void* grid_ws; int64_t grid_n_max;
  const float* views; int n_views; float znear; float zfar; int backface_culling;
  int32_t* mask_out; void* front_ws; int64_t front_ws_bytes;
  int64_t* first_idx_out; int64_t* num_pts_out; int32_t* view_total_out;
} iso_follow;

/* iso_project_sphere + the side work described by *follow (a HOST struct, read during the call). */
int iso_project_sphere_follow(const float* pts_in, float* pts_out, float* normals_out,
                              uint8_t* mask_out, int64_t n, float cx, float cy,
                              float cz, float radius, int max_iters, float tol,
                              const iso_follow* follow_host, void* stream);

/* SIREN SDF (DSS/models/common.py:90-165): dims 3 -> H -> (H)*n_hidden -> 1,
 * h0 = sin(w0*(W0 x+b0)), hi = sin(w*(Wi h+bi)), sdf = WL h + bL.
 * Weights are handed over exactly as torch stores them (row-major
 * [out][in]) in ONE packed f32 buffer:
 *   W0[H*3] b0[H]  { Wi[H*H] bi[H] } * n_hidden   WL[H] bL[1]
 * iso_siren_pack_weights() re-orders the hidden matrices into the MFMA
 * lane-linear images the projection kernel streams (forward + transposed).
 * H must be a multiple of 16, 16 <= H <= 512; 0 <= n_hidden <= 8.            */
int64_t iso_siren_raw_floats(int hidden, int n_hidden);
int64_t iso_siren_packed_floats(int hidden, int n_hidden);
int iso_siren_pack_weights(const float* raw, float* packed, int hidden,
                           int n_hidden, void* stream);
/* How the H x H products of the hidden layers are formed (process-wide switch):
 *   1 (default)  fp16 matrix cores at f32 accuracy: every f32 operand is cut into two fp16
 *                numbers (11 + 11 significant bits) under an exact power-of-two scale -- per layer
 *                for the weights, 2^12 for the activations, per point for the adjoint of the reverse
 *                sweep -- and three partial products are accumulated in f32: same error level as an
 *                f32 GEMM (the accumulation dominates), 5.3x the MFMA rate.  H in {128,256},
 *                n_hidden >= 1.
 *   0            f32 matrix cores (v_mfma_f32_16x16x4_f32: a sum over the H inputs is two fmaf chains, over the even and
 *                the odd chunks of 16 inputs, added at the end).
 * Shapes mode 1 does not cover run in mode 0.  ISO_SIREN_GEMM=f32 in the environment selects 0. */
int iso_siren_set_gemm_mode(int mode);
int iso_siren_get_gemm_mode(void);
/* Newton tail of iso_project_siren (H = 256, split-fp16 mode): the iterations from `first_tail_iteration` on run as ONE
 * launch whose workgroups iterate the survivors of their own tiles until none is left (the reference leaves its loop
 * when nothing is active, levelset_sampling.py:329) -- instead of one launch per iteration, most of them for a few
 * hundred points or none.  -1: the default (4 for max_iters >= 6, else 2), 0: never (a launch per iteration), k >= 1.
 * Results do not depend on it (a point's evaluation does not depend on the tile it sits in).              */
int iso_siren_set_tail_from(int first_tail_iteration);
/* Which tile a workgroup of the step kernels takes next: drawn from a per-launch counter (1, the default: the XCDs of one
 * GPU do not run alike under the power cap, equal static shares end with the slowest) or every gridDim-th (0).  -1: back to
 * the default.  Results do not depend on it. */
int iso_siren_set_drawn_tiles(int on);
int iso_idr_set_drawn_tiles(int on);
/* Form of the split-fp16 gradient step at hidden size 256.  1 (the default): four waves per workgroup, one per SIMD with
 * 512 registers each, the derivative stash of the reverse sweep held in LDS and registers -- for n_hidden 2 and 3; every
 * other shape, forward-only evaluation, latent-coded networks (iso_*_siren_coded) and the f32 mode keep their kernels.  0: eight waves, the stash in global memory
 * (the workspace keeps room for it either way).  Results do not depend on it, bit for bit.
 * iso_siren_step_form_used: the form that serves a gradient step of this shape (coded != 0: of a coded network) as
 * things are set now. */
int iso_siren_set_step_form(int form);
int iso_siren_get_step_form(void);
int iso_siren_step_form_used(int hidden, int n_hidden, int coded);
/* Which step kernel serves a call of this shape as the GEMM mode and the step form are set now (host only, nothing is
 * launched).  value_only != 0: sphere tracing, or iso_siren_sdf_grad without grad_out; coded != 0: an iso_*_siren_coded entry.
 *   100 + H/16  k_siren_step<H/16, coded>                      mode 0; or H = 64; or n_hidden = 0
 *   200 + H/16  k_siren_step_x3<H, ., ., ., true, coded>       mode 1, H = 128 / 256, n_hidden 1..8, value only
 *   308         k_siren_step_x3<128, 4, 3, 1, false, coded>    mode 1, H = 128, n_hidden 1..8, gradient
 *   416         k_siren_step_x3_both<256, 8, 3, 1, coded>      mode 1, H = 256, n_hidden 1..8, gradient, unless 516
 *   516         k_siren_step_x3_both_oc<256, 3, 1, false, L>   mode 1, step form 1, H = 256, n_hidden 2 / 3, gradient, uncoded
 *   -1          H not 64 / 128 / 256 or n_hidden outside 0..8
 * The Newton tail (iso_siren_set_tail_from) and the drawn tiles (iso_siren_set_drawn_tiles) go with 416 and 516 alone;
 * iso_siren_step_form_used is "the gradient step's code is 516". */
int iso_siren_step_kernel(int hidden, int n_hidden, int value_only, int coded);
/* step-kernel launches one iso_project_siren call with these arguments issues (max_iters + 1 without the tail) */
int iso_siren_step_launches(int hidden, int n_hidden, int max_iters);
/* scratch for the per-wave activation-derivative stash */
int64_t iso_project_siren_workspace_bytes(int64_t n, int hidden, int n_hidden);
/* diagnostics: byte offset, inside that workspace, of the 64 int32 counters a projection leaves behind -- [it] = points
 * evaluated by iteration it (it >= 1; iteration 0 evaluates all n) */
int64_t iso_project_siren_counts_offset(int64_t n, int hidden, int n_hidden);
int iso_project_siren(const float* pts_in, float* pts_out, float* normals_out,
                      uint8_t* mask_out, int64_t n, const float* packed,
                      int hidden, int n_hidden, float omega_first,
                      float omega_hidden, int max_iters, float tol,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* one SDF + gradient evaluation, no Newton move (used by tests and by callers
 * that only need _compute_sdf_and_grad, levelset_sampling.py:142-170).
 * grad_out may be NULL: value only, the reverse sweep is skipped (the `sdf` callable of
 * RayTracing, levelset_sampling.py:831-1167, and the candidate evaluations of
 * combined_modeling.py:376-380).                                              */
int iso_siren_sdf_grad(const float* pts, float* sdf_out, float* grad_out,
                       int64_t n, const float* packed, int hidden,
                       int n_hidden, float omega_first, float omega_hidden,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Latent-conditioned SIREN (the reference's Siren(c_dim = C), DSS/models/common.py:90-165: forward concatenates the
 * code in front of the point, [c, x], :150-152; its callers pass one code per cloud / batch row: combined_modeling.py:449,
 * implicit_modeling.py:156-159 (projection), :305,313 (sphere tracing), :318-319 (secant search)).  Layer 0 of code u is
 * sin(w0 (W0[:, C:] x + b_u)) with b_u = b0 + W0[:, :C] c_u: only layer 0's bias depends on the code.
 * iso_siren_fold_codes: table[u * padded_hidden + f] = b0[f] + sum_k w0c[f * c_dim + k] codes[u * c_dim + k] for
 *   f < hidden (accumulated in double in the order b0, k = 0, 1, ..; rounded once), 0 for hidden <= f < padded_hidden.
 *   w0c = W0[:, :C] row-major (hidden x c_dim), b0 (hidden), codes (n_codes x c_dim); table (n_codes x padded_hidden) f32.
 * The *_coded entry points take the image of the network whose W0 is W0[:, C:] (iso_siren_pack_weights; its b0 is not
 * read) plus the table (padded_hidden = `hidden` of the call) and code_of (n int32, the table row of point / ray i, each
 * in [0, n_codes); NULL: row 0 for every point, n_codes must then be 1).  A coded evaluation with row u is bit-identical
 * to the uncoded one of the network whose b0 is row u.                                                               */
int iso_siren_fold_codes(const float* w0c, const float* b0, const float* codes, float* table, int hidden,
                         int padded_hidden, int c_dim, int64_t n_codes, void* stream);
int iso_project_siren_coded(const float* pts_in, float* pts_out, float* normals_out,
                            uint8_t* mask_out, int64_t n, const float* packed,
                            int hidden, int n_hidden, float omega_first,
                            float omega_hidden, int max_iters, float tol,
                            void* workspace, int64_t workspace_bytes, void* stream,
                            const float* code_bias, const int32_t* code_of, int64_t n_codes);
int iso_siren_sdf_grad_coded(const float* pts, float* sdf_out, float* grad_out,
                             int64_t n, const float* packed, int hidden,
                             int n_hidden, float omega_first, float omega_hidden,
                             void* workspace, int64_t workspace_bytes, void* stream,
                             const float* code_bias, const int32_t* code_of, int64_t n_codes);

/* IDR-style SDF (DSS/models/common.py:220-310): positional encoding with n_freq
 * frequencies (D0 = 3 + 6*n_freq <= 63), n_layers softplus(beta) layers of width `hidden`
 * (128/256/512), optional skip connection [h, e(x)]/sqrt(2) into layer skip_layer (< 0: none;
 * layer skip_layer-1 is then hidden-D0 wide), linear head, tanh.  Weight-norm must already be
 * folded into the weights.  raw = for l = 0..n_layers: W_l (row-major [out][in]) then b_l.
 * hidden 256 / 512 with n_freq <= 6 run on the fp16 matrix cores at f32 accuracy (two fp16 parts
 * per operand under exact power-of-two scales, as iso_siren_set_gemm_mode(1)); ISO_IDR_GEMM=f32 in
 * the environment, hidden 128 and wider encodings use the f32 matrix cores.
 *
 * iso_idr_set_gemm_mode: 1 (the default) = split fp16 where it applies, 0 = the f32 matrix cores for every shape; any other
 *   value is ISO_ERR_INVALID.  The initial value is 0 when ISO_IDR_GEMM=f32 is in the environment.  The mode may change
 *   between two calls on the same packed buffer and workspace: both hold what either form needs.
 * iso_idr_step_form (host only, no GPU): the step kernel a call with this shape takes under the current mode, by the
 *   predicates the launch itself uses.  value_only = 0: iso_project_idr and iso_idr_sdf_grad with grad_out; value_only = 1:
 *   iso_trace_idr and iso_idr_sdf_grad with grad_out = NULL.  NT = hidden / 16, D0 = 3 + 6 n_freq:
 *     400 + NT  k_idr_step_x16<hidden, ., false>   hidden 256 / 512, D0 <= 39 (n_freq <= 6), mode 1, value_only = 0
 *     500 + NT  k_idr_step_x16<hidden, ., true>    the same, value_only = 1
 *     200 + NT  k_idr_step_fs<NT, false>           otherwise: hidden 256 / 512, D0 <= 48 (n_freq <= 7), value_only = 0
 *     300 + NT  k_idr_step_fs<NT, true>            otherwise: D0 <= 48, value_only = 1 (hidden 128 included)
 *     100 + NT  k_idr_step<NT> (staged)            otherwise: hidden 128 with value_only = 0, and every D0 > 48 (n_freq >= 8)
 *     -1        a shape the entry points refuse (ISO_ERR_UNSUPPORTED)                                                   */
int iso_idr_set_gemm_mode(int mode);
int iso_idr_get_gemm_mode(void);
int iso_idr_step_form(int hidden, int n_layers, int skip_layer, int n_freq, int value_only);
int64_t iso_idr_raw_floats(int hidden, int n_layers, int skip_layer, int n_freq);
int64_t iso_idr_packed_floats(int hidden, int n_layers);
int iso_idr_pack_weights(const float* raw, float* packed, int hidden, int n_layers,
                         int skip_layer, int n_freq, void* stream);
int64_t iso_project_idr_workspace_bytes(int64_t n, int hidden, int n_layers);
int iso_project_idr(const float* pts_in, float* pts_out, float* normals_out, uint8_t* mask_out,
                    int64_t n, const float* packed, int hidden, int n_layers, int skip_layer,
                    int n_freq, float beta, int max_iters, float tol, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* grad_out may be NULL (value only, forward sweep only). */
int iso_idr_sdf_grad(const float* pts, float* sdf_out, float* grad_out, int64_t n,
                     const float* packed, int hidden, int n_layers, int skip_layer, int n_freq,
                     float beta, void* workspace, int64_t workspace_bytes, void* stream);

/* Sphere tracing along given rays: SphereTracing.project_points,
 * DSS/models/levelset_sampling.py:679-808 (callers implicit_modeling.py:305,313).
 *   p_0 = ray0; per iteration (max_iters advances, max_iters + 1 evaluations):
 *     f = sdf(p)                                       value only -- the gradient the reference
 *                                                      computes at :745-757 is never used (:806)
 *     still active: |f| > 0.1 * tol  and  inside       (:764)
 *     m = (alpha f) d;  m = m / max(|m|,1e-15) * min(|m|,0.1);  q = p + m        (:771-775)
 *     inside = |q| < bound (= radius + padding);  p = q only while inside        (:776-779)
 *   outputs: pts_out (n,3) the last position inside the bounding sphere, sdf_out (n) the value at
 *   it (`network_eval_on_levelset_points`), mask_out (n) = |sdf| <= tol (:790).
 *   dirs (n,3) are the (normalised) ray directions.  One launch per iteration over a device-side
 *   active list, as iso_project_*; workspaces are those of iso_project_siren / iso_project_idr. */
int iso_trace_sphere(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                     uint8_t* mask_out, int64_t n, float cx, float cy, float cz, float radius,
                     float alpha, float bound, int max_iters, float tol, void* stream);
int iso_trace_siren(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                    uint8_t* mask_out, int64_t n, const float* packed, int hidden, int n_hidden,
                    float omega_first, float omega_hidden, float alpha, float bound, int max_iters,
                    float tol, void* workspace, int64_t workspace_bytes, void* stream);
/* the same for a latent-conditioned SIREN (implicit_modeling.py:305,313: SphereTracing.project_points(latent=c)); the
 * code arguments as iso_project_siren_coded, code_of indexed by ray */
int iso_trace_siren_coded(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                          uint8_t* mask_out, int64_t n, const float* packed, int hidden, int n_hidden,
                          float omega_first, float omega_hidden, float alpha, float bound, int max_iters,
                          float tol, void* workspace, int64_t workspace_bytes, void* stream,
                          const float* code_bias, const int32_t* code_of, int64_t n_codes);
int iso_trace_idr(const float* ray0, const float* dirs, float* pts_out, float* sdf_out,
                  uint8_t* mask_out, int64_t n, const float* packed, int hidden, int n_layers,
                  int skip_layer, int n_freq, float beta, float alpha, float bound, int max_iters,
                  float tol, void* workspace, int64_t workspace_bytes, void* stream);

/* Texture network, forward only: RenderingNetwork.forward, DSS/models/common.py:351-366, on the rows NeuralTexture.forward
 * builds (DSS/core/texture.py:136-159); reached by ImplicitModel.decode_color (implicit_modeling.py:96-113),
 * Generator.estimate_colors (:790-820) and Generator.raytrace_images (:951-1001).
 *   x_i  = [ codes_i (c_dim) | normal_i, point_i (geom = 6) or point_i (geom = 3) | e(d_i) (n_freq >= 0) ]
 *   d_i  = v / max(|v|, 1e-12),  v = point_i - view_origins[origin_of[i]]             (F.normalize, texture.py:152-153)
 *   e(d) = [d, sin(2^0 d), cos(2^0 d), ..., sin(2^(F-1) d), cos(2^(F-1) d)], 3 + 6 F slots (get_embedder :205-217); F = 0:
 *          the raw direction; n_freq = -1: no view direction, no slots
 *   h_0  = relu(W_0 x + b_0),  h_l = relu(W_l h_(l-1) + b_l), l < n_layers;  rgb = (tanh(W_n h + b_n) + 1) / 2    (:356-365)
 * Shape (hidden, n_layers, c_dim, geom, n_freq): hidden 256 / 512, 1 <= n_layers <= 8, 0 <= c_dim <= 256, geom 3 / 6,
 * -1 <= n_freq <= 6, three outputs; the row is D0 = c_dim + geom + (3 + 6 n_freq) <= 301 long.  Weight-norm must already be
 * folded into the weights.  raw = for l = 0..n_layers: W_l (row-major [out][in]) then b_l.
 * One persistent kernel per hidden size on the fp16 matrix cores at f32 accuracy (two fp16 parts per operand under exact
 * power-of-two scales, per layer for the weights and per point for the activations and the input row); the row is
 * assembled in the kernel, no (n, D0) matrix is written.
 *
 * iso_texture_form (host only, no GPU): 600 + hidden / 16 = k_texture_x16<hidden>, by the predicate the packing and the
 *   launch use; -1: a shape they refuse (ISO_ERR_UNSUPPORTED).
 * iso_texture_raw_floats / iso_texture_packed_floats: lengths of raw and packed (0 for a refused shape).
 * iso_texture_rgb: points (n,3); normals (n,3), NULL iff geom == 3; codes (n, c_dim), NULL iff c_dim == 0; view_origins
 *   (n_origins, 3), NULL iff n_freq < 0; origin_of (n) int32 in [0, n_origins), NULL = origin 0 for every point; rgb_out
 *   (n,3) in [0, 1].  A point's result does not depend on the other points of the call.  Refusals launch nothing: an
 *   unsupported shape is ISO_ERR_UNSUPPORTED; a NULL pointer where one is required, one given where none is allowed, and a
 *   workspace below iso_texture_workspace_bytes are ISO_ERR_INVALID; n == 0 is ISO_OK without a launch.              */
int iso_texture_form(int hidden, int n_layers, int c_dim, int geom, int n_freq);
int64_t iso_texture_raw_floats(int hidden, int n_layers, int c_dim, int geom, int n_freq);
int64_t iso_texture_packed_floats(int hidden, int n_layers, int c_dim, int geom, int n_freq);
int iso_texture_pack_weights(const float* raw, float* packed, int hidden, int n_layers, int c_dim, int geom,
                             int n_freq, void* stream);
int64_t iso_texture_workspace_bytes(int64_t n, int hidden, int n_layers, int c_dim, int geom, int n_freq);
int iso_texture_rgb(const float* points, const float* normals, const float* codes, const float* view_origins,
                    const int32_t* origin_of, int64_t n_origins, float* rgb_out, int64_t n, const float* packed,
                    int hidden, int n_layers, int c_dim, int geom, int n_freq, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* Backward of the texture network (csrc/texgrad.hip): given g = dL/d rgb (n,3), the gradient of every weight and bias
 * and of the codes, normals and points of the rows.  With z_l = W_l h_(l-1) + b_l, h_l = relu(z_l), y = W_n h + b_n:
 *   dy  = g (1 - tanh^2 y) / 2,  dW_n = dy^T h,  db_n = sum_p dy,  a_top = (W_n^T dy) [z_top > 0]
 *   dW_l = a_l^T h_(l-1),  db_l = sum_p a_l,  a_(l-1) = (W_l^T a_l) [z_(l-1) > 0],  dW_0 = a_0^T x
 *   dx = W_0^T a_0, cut into d codes | d normals | d points; the view slots are dropped (the reference detaches the
 *   direction, texture.py:152) and the view origins get no gradient.  The ReLU mask is zero at z == 0, as torch's.
 * Same shapes as iso_texture_*.  Two kernels per 64-point tile on the fp16 matrix cores at f32 accuracy: the forward's own
 * form recomputes and stashes every h_l (k_texgrad_fwd_x16<hidden>), and the reverse sweep runs the same three-pass GEMM on
 * transposed split-fp16 images, the adjoint cut under a per-point power-of-two scale from the column-sum bound
 * (k_texgrad_rev_x16<hidden>).  The head adjoint, dx and the dW products run in f32 (dx and dW on the exact f32 matrix
 * instruction).  The
 * reduction over the points is cut into chunks of iso_texgrad_chunk_points() points BY INDEX, one partial per chunk, the
 * partials added in chunk order: no float atomic, the same bits on every call.  A point's d codes / d normals / d points
 * do not depend on the other points of the call.
 *
 * iso_texgrad_form (host only): 700 + hidden / 16 for an accepted shape (one code per width, as iso_texture_form's
 *   600 + hidden / 16), -1 for a refused one.
 * iso_texgrad_packed_floats / iso_texgrad_pack_weights: the backward's own image of raw (iso_texture_raw_floats), separate
 *   from the forward's packed image, which the recompute reads unchanged: per-layer weight scales and column sums, the
 *   head rows and bias, W_0^T in f32 and the split-fp16 images of W_l^T, l >= 1.  Its layout is private to the library and
 *   its length is whatever iso_texgrad_packed_floats returns: size the buffer by that call, not by a formula.
 * iso_texgrad_workspace_points (host only) / iso_texgrad_workspace_bytes: the points are processed
 *   iso_texgrad_workspace_points() = 16384 at a time, so the workspace stops growing there:
 *   4 * (mw * (K0 + 2 * n_layers * hidden + 4) + ceil(mw / chunk_points) * raw_floats) + 64, mw = min(max(n, 1), 16384),
 *   K0 = D0 rounded up to a multiple of 64.
 * Summation: dW_l partials are f32 matrix-instruction chains over the 512 points of a chunk; db_l, dW_n and db_n add
 *   their terms in float64 and round to f32 once per chunk; the partials of one workspace chunk (up to 32) are added in
 *   chunk order in ONE float64 chain and rounded to f32 once, on top of the f32 sum of the earlier workspace chunks.
 * iso_texgrad_backward: inputs as iso_texture_rgb, grad_rgb (n,3); packed_fw the forward's image of the same weights
 *   (iso_texture_pack_weights), packed_bw the backward's; grad_raw_out in the layout of raw, NULL = the weight gradients
 *   are not wanted (no dW / db work is done); grad_points (n,3), grad_normals (n,3), grad_codes (n, c_dim): each may be
 *   NULL (not wanted; all three NULL skips dx); grad_normals / grad_codes must be NULL where the shape has no normals /
 *   codes.  Outputs are written, not accumulated.  Refusals as iso_texture_rgb, launching nothing; workspace, packed_fw
 *   and packed_bw must be 16-byte aligned; n == 0 writes zeros to grad_raw_out and is ISO_OK.                          */
int iso_texgrad_form(int hidden, int n_layers, int c_dim, int geom, int n_freq);
int64_t iso_texgrad_packed_floats(int hidden, int n_layers, int c_dim, int geom, int n_freq);
int iso_texgrad_pack_weights(const float* raw, float* packed_bw, int hidden, int n_layers, int c_dim, int geom,
                             int n_freq, void* stream);
int64_t iso_texgrad_chunk_points(void);
int64_t iso_texgrad_workspace_points(void);
int64_t iso_texgrad_workspace_bytes(int64_t n, int hidden, int n_layers, int c_dim, int geom, int n_freq);
int iso_texgrad_backward(const float* points, const float* normals, const float* codes, const float* view_origins,
                         const int32_t* origin_of, int64_t n_origins, const float* grad_rgb, int64_t n,
                         const float* packed_fw, const float* packed_bw, int hidden, int n_layers, int c_dim, int geom, int n_freq,
                         float* grad_raw_out, float* grad_points, float* grad_normals, float* grad_codes,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* Backward of the SIREN SDF AND of its gradient (csrc/sirengrad.hip): given u = dL/d sdf (n) and v = dL/d grad (n,3) of
 * one iso_siren_sdf_grad evaluation, the gradient of every weight and bias and of the points.  With u, v held constant this
 * is the derivative of u f + v . grad f, and v . grad f is the forward-mode derivative of f along v: one tangent column per
 * point (s_l = w cos(w z_l)):
 *   zt_0 = W_0 v, ht_l = s_l zt_l, zt_l = W_l ht_(l-1);  dw_L = sum_p (u h_top + ht_top), db_L = sum_p u
 *   ztbar_l = htbar_l s_l, zbar_l = hbar_l s_l - w^2 h_l zt_l htbar_l   (seeds hbar_top = u w_L, htbar_top = w_L)
 *   dW_l = sum_p (zbar_l h_(l-1)^T + ztbar_l ht_(l-1)^T), db_l = sum_p zbar_l, hbar_(l-1) = W_l^T zbar_l, htbar_(l-1) = W_l^T ztbar_l
 *   dW_0 = sum_p (zbar_0 x^T + ztbar_0 v^T), d pts = W_0^T zbar_0
 * All matrix products run on the exact f32 matrix instruction, whatever iso_siren_set_gemm_mode says: the sweeps are the f32
 * tile GEMM of the step kernel (k_siren_step's) on the f32 weight images inside `packed`, a wave's 16 columns being 8 points
 * x {value, tangent} (k_sirengrad_sweep<hidden / 16, tangent>); dW_l is one product over 2 n rows (k_sirengrad_tn).  The
 * reduction over the points is cut into chunks of iso_sirengrad_chunk_points() = 256 points BY INDEX: dW_l partials are f32
 * matrix-instruction chains over a chunk's rows; db_l, dW_0, dw_L and db_L add exact products in float64 and round to f32
 * once per chunk (k_sirengrad_cols); the partials of one workspace chunk are added in chunk order in ONE float64 chain and
 * rounded to f32 once, on top of the f32 sum of the earlier workspace chunks (k_grad_reduce).  No float atomic, the same
 * bits on every call; a point's d pts does not depend on the other points of the call.
 *
 * iso_sirengrad_form (host only): 800 + H / 16, H the kernel width that serves a network of `hidden` units (64 / 128 / 256,
 *   the next one up: the caller zero-pads), for 1 <= hidden <= 256 and 0 <= n_hidden <= 8; 0 for a shape that is refused.
 * iso_sirengrad_workspace_points / iso_sirengrad_workspace_bytes (host only): the points are processed
 *   iso_sirengrad_workspace_points() = 16384 at a time, so the workspace stops growing there:
 *   4 * (256 + 4 * (n_hidden + 1) * mw * hidden + ceil(mw / chunk_points) * raw_floats), mw = min(max(n, 1), 16384);
 *   0 for a shape iso_sirengrad_backward refuses.
 * iso_sirengrad_backward: pts (n,3), g_sdf (n), g_grad (n,3) or NULL (only the value was used: the first-order form, 16
 *   value columns per wave, no tangent work); packed from iso_siren_pack_weights of the same weights, `hidden` its width
 *   (64 / 128 / 256 exactly: ISO_ERR_UNSUPPORTED otherwise, as n_hidden outside 0..8); raw is the vector packed was made
 *   from and is not read by this version (it may be NULL).  grad_raw_out in the layout of raw (iso_siren_raw_floats), NULL =
 *   the weight gradients are not wanted (no dW / db work is done); grad_pts_out (n,3) or NULL.  Outputs are written, not
 *   accumulated; zero-padded rows and columns of the weights get zero gradients.  n < 0, a NULL pts / g_sdf / packed /
 *   workspace, and a workspace or packed that is not 16-byte aligned are ISO_ERR_INVALID; a workspace below
 *   iso_sirengrad_workspace_bytes is ISO_ERR_WORKSPACE; nothing is launched on a refusal.  n == 0 writes zeros to
 *   grad_raw_out and is ISO_OK.
 * iso_sirengrad_backward_b0: the same call with layer 0's bias b_0[f] = packed's b_0[f] + b0_tail[f] (hidden floats in natural
 *   feature order, NULL = none), the sum taken in float64 inside z_0.  For a latent-conditioned SIREN, whose code is folded
 *   into b_0 (iso_siren_fold_codes: b_0 + W_0[:, :C] c): the f32 rounding of the folded bias is the SAME for every point, so
 *   unlike a per-point rounding it does not average out of the sums over the points; the caller hands over the bits the
 *   f32 bias lost (sdf_models.siren_forward).  grad_raw_out's b_0 is the gradient of the whole bias.                       */
int iso_sirengrad_form(int hidden, int n_hidden);
int64_t iso_sirengrad_workspace_points(void);
int64_t iso_sirengrad_chunk_points(void);
int64_t iso_sirengrad_workspace_bytes(int64_t n, int hidden, int n_hidden);
int iso_sirengrad_backward(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* raw,
                           const float* packed, int hidden, int n_hidden, float omega_first, float omega_hidden,
                           float* grad_raw_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes, void* stream);
int iso_sirengrad_backward_b0(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* raw,
                              const float* packed, int hidden, int n_hidden, float omega_first, float omega_hidden,
                              float* grad_raw_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes, void* stream,
                              const float* b0_tail);

/* The same backward with ONE LATENT CODE PER CLOUD: the auto-decoder training step of the reference's default decoder,
 * Siren(c_dim = 256) (config.py:163-166), whose multi-shape callers gather one code per packed point
 * (implicit_modeling.py:190-218: get_normals_from_grad on packed points with the codes taken by packed_to_cloud_idx).
 * Only layer 0's bias depends on the code: z_0(p) = W0x x_p + t_u(p), t_u = b_0 + W0c c_u one row of a table per code
 * (iso_siren_fold_codes).  The new output is the table's gradient dt_u = sum over the points of row u of zbar_0(p); the
 * caller's chain over the fold gives d c_u = W0c^T dt_u, d W0c = sum_u dt_u c_u^T and d b_0 = sum_u dt_u.
 * The points of a row are CONTIGUOUS: point p belongs to row u iff code_first[u] <= p < code_first[u + 1].  dt_u is
 * summed in float64 over the same fixed 256-point pieces (and their quarters) as every other sum here, a partial per piece
 * and row rounded to f32 once, the partials of a row added in piece order in one float64 chain per workspace chunk on top
 * of the earlier chunks (k_sirencode_rows, k_sirencode_join): no float atomic, the same bits on every call, a long row is
 * spread over the grid.  A row without points gets zeros.
 *
 * iso_sirencode_workspace_bytes (host only): iso_sirengrad_workspace_bytes(n, hidden, n_hidden) + 4 * 2 * hidden *
 *   ceil(mw / 256), mw = min(max(n, 1), 16384) -- two partial rows per piece, placed after the uncoded layout; it does not
 *   grow with n_codes.  0 for a shape that is refused and for n_codes < 1.
 * iso_sirencode_backward: pts, g_sdf, g_grad or NULL, n, hidden, n_hidden and the omegas as iso_sirengrad_backward; packed
 *   the image of the network whose W_0 is W0x (its b_0 is not read).  code_bias (n_codes, hidden) f32, the table, in natural
 *   feature order; code_tail the same shape or NULL: the bits each row lost when it was rounded to f32, added in float64
 *   inside z_0 (iso_sirengrad_backward_b0's tail, per row); code_of (n) int32 the row of every point, clamped into
 *   [0, n_codes) before it is used; code_first (n_codes + 1) int64 ON THE DEVICE, every value read clamped into [0, n]; the
 *   two must describe the same rows.  grad_raw_out (layout of iso_siren_raw_floats; its W_0 is d W0x and its b_0 the sum
 *   over ALL points) or NULL, grad_code_bias_out (n_codes, hidden) or NULL, grad_pts_out (n,3) or NULL: NULL outputs select
 *   the work; outputs are written, not accumulated; padded features get zeros.  With n_codes = 1 every output has the
 *   bits of iso_sirengrad_backward_b0 run with row 0 as b_0 and tail.  Refusals as iso_sirengrad_backward, nothing launched:
 *   shape ISO_ERR_UNSUPPORTED; n < 0, n_codes < 1, a NULL pts / g_sdf / packed / workspace / code_bias / code_of /
 *   code_first, a workspace, packed, code_bias or code_tail that is not 16-byte aligned ISO_ERR_INVALID; a workspace below
 *   iso_sirencode_workspace_bytes ISO_ERR_WORKSPACE.  n == 0 writes zeros to the outputs asked for except grad_pts_out.  */
int64_t iso_sirencode_workspace_bytes(int64_t n, int hidden, int n_hidden, int64_t n_codes);
int iso_sirencode_backward(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* packed, int hidden,
                           int n_hidden, float omega_first, float omega_hidden, const float* code_bias, const float* code_tail,
                           const int32_t* code_of, const int64_t* code_first, int64_t n_codes, float* grad_raw_out,
                           float* grad_code_bias_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes, void* stream);

/* Backward of the IDR SDF AND of its gradient (csrc/idrgrad.hip): given u = dL/d sdf (n) and v = dL/d grad (n,3) of one
 * iso_idr_sdf_grad evaluation, the gradient of every EFFECTIVE weight and bias and of the points.  As iso_sirengrad_backward:
 * with u, v held constant this is the derivative of u f + v . grad f, one tangent column per point:
 *   et_k = dval_k v_c(k), zt_l = W_l int_l, s_l = sigmoid(beta z_l), ht_l = s_l zt_l, int_skip = [ht_(skip-1); et] / sqrt(2)
 *   yt = w_n . ht_(n-1), d = 1 - f^2;  ybar = d (u - 2 f yt), ytbar = d;  dw_n = sum_p (ybar h_(n-1) + ytbar ht_(n-1)), db_n = sum_p ybar
 *   ztbar_l = htbar_l s_l, zbar_l = hbar_l s_l + htbar_l zt_l s'_l, s'_l = beta s_l (1 - s_l)   (seeds ybar w_n, ytbar w_n)
 *   dW_l = sum_p (zbar_l in_l^T + ztbar_l int_l^T), db_l = sum_p zbar_l, inbar_l = W_l^T zbar_l, intbar_l = W_l^T ztbar_l
 *   d pts_c = sum over the encoding slots k of coordinate c of (ebar_k dval_k + etbar_k d2val_k v_c)
 * All matrix products run on the exact f32 matrix instruction, whatever iso_idr_set_gemm_mode says: the sweeps are the staged
 * f32 tile GEMM on the FW / BW / FW0 / W0v images inside `packed`, a wave's 16 columns being 8 points x {value, tangent}
 * (k_idrgrad_sweep<hidden / 16, tangent>, one workgroup per CU, 160 KiB of LDS at hidden 512); dW_l is one product over 2 n
 * rows (k_grad_tn; dW_0 on a 64-wide stash of the encoding).  The reduction over the points is cut into chunks of
 * iso_idrgrad_chunk_points() = 256 points BY INDEX: dW_l partials are f32 matrix-instruction chains over a chunk's rows; db_l,
 * dw_n and db_n add exact products in float64 and round to f32 once per chunk (k_idrgrad_cols); the partials of one workspace
 * chunk are added in chunk order in ONE float64 chain and rounded to f32 once, on top of the f32 sum of the earlier workspace
 * chunks (k_grad_reduce).  No float atomic, the same bits on every call; a point's d pts does not depend on the other
 * points of the call.
 *
 * iso_idrgrad_form (host only): 900 + hidden / 16 for every shape iso_idr_pack_weights accepts (hidden 128 / 256 / 512, 2..12
 *   layers, n_freq <= 10, skip_layer < 0 or in 1 .. n_layers - 1); 0 for a shape that is refused.
 * iso_idrgrad_workspace_points / iso_idrgrad_workspace_bytes (host only): the points are processed
 *   iso_idrgrad_workspace_points() = 8192 at a time (one 32-point tile for each of 256 workgroups), so the workspace stops
 *   growing there.  In floats, with mw = min(max(n, 1), 8192):
 *     512 zeros | 2 mw * 64 encoding stash | n_layers * 2 mw * hidden input stash (in_1 .. in_(n-1), h_(n-1)) |
 *     n_layers * 2 mw * hidden derivative stash (s_l | zt_l s'_l, then zbar_l | ztbar_l) | 2 mw head | ceil(mw / 256) * raw_floats
 *   every stash row-major, row 2 p the value row of point p and row 2 p + 1 its tangent row (row p without g_grad).  For the
 *   reference's 8 x 512, skip 4, 6 frequencies that is 776 598 784 bytes from 8192 points on; 0 for a refused shape.
 * iso_idrgrad_backward: pts (n,3), g_sdf (n), g_grad (n,3) or NULL (only the value was used: the first-order form, 16 value
 *   columns per wave, no tangent work); packed from iso_idr_pack_weights of the same weights; raw is the vector packed was
 *   made from and is not read by this version (it may be NULL); beta must be 100.  grad_raw_out in the layout of raw
 *   (iso_idr_raw_floats: the narrow layer at its true hidden - D0 rows), NULL = the weight gradients are not wanted (no dW / db
 *   work is done); grad_pts_out (n,3) or NULL; both NULL: nothing is launched.  Outputs are written, not accumulated.  An
 *   unsupported shape or beta is ISO_ERR_UNSUPPORTED; n < 0, a NULL pts / g_sdf / packed / workspace, and a workspace or
 *   packed that is not 16-byte aligned are ISO_ERR_INVALID; a workspace below iso_idrgrad_workspace_bytes is
 *   ISO_ERR_WORKSPACE; nothing is launched on a refusal.  n == 0 writes zeros to grad_raw_out and is ISO_OK.               */
int iso_idrgrad_form(int hidden, int n_layers, int skip_layer, int n_freq);
int64_t iso_idrgrad_workspace_points(void);
int64_t iso_idrgrad_chunk_points(void);
int64_t iso_idrgrad_workspace_bytes(int64_t n, int hidden, int n_layers, int skip_layer, int n_freq);
int iso_idrgrad_backward(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* raw,
                         const float* packed, int hidden, int n_layers, int skip_layer, int n_freq, float beta,
                         float* grad_raw_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes, void* stream);

/* Nearest point to each ray (brute force, fused): the (R,M) point-to-ray search of
 * CombinedModel.sample_offsurface_using_isopoints, DSS/models/combined_modeling.py:336-352.
 *   pC = p - origin;  ray_sq = (pC . ray)^2;  dist = |pC|^2 - ray_sq;  nn = argmin_m dist
 *   idx_out (R) i32 = nn (lowest index among equal distances; -1 when there are no points),
 *   raysq_out (R) = ray_sq[r, nn] (the reference's `ray_len` before eps_sqrt().sqrt(), :345,:353),
 *   dist_out (R, may be NULL) = dist[r, nn].  rays (R,3) unit directions, points (M,3).       */
int64_t iso_ray_nearest_point_workspace_bytes(int64_t n_rays);
int iso_ray_nearest_point(const float* rays, int64_t n_rays, float ox, float oy, float oz,
                          const float* points, int64_t n_points, int32_t* idx_out,
                          float* raysq_out, float* dist_out, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* State updates of IDR's two-ended ray marcher between two network evaluations
 * (RayTracing.sphere_tracing / .secant, DSS/models/levelset_sampling.py:920-1032, :1114-1133).
 * Per ray two marching ends: arrays of shape (2,R) hold end 0 (forward from the bounding-sphere
 * entry) in [0,R) and end 1 (backward from the exit) in [R,2R).  cam, dirs (R,3) are the ray
 * origin and unit direction.  Each call writes `list` (<= 2R,3): the points that need a network
 * value next, `slot` (2,R) i32: their position in the list (-1: none), and `*count` (device i32):
 * how many there are -- the caller reads it, evaluates list[0:count] and passes the values on.
 *
 * iso_raymarch_settle (:962-990 and, with check_order, the z0 < z1 test of :1027-1030 that ends
 *   the previous iteration): cur = live ? nxt : 0;  cur <= thr -> 0;  live &= cur > thr;
 *   *count = unfinished ends; when `step`: z0 += cur0, z1 -= cur1, list <- cam + z d of those ends.
 * iso_raymarch_overshoot (:993-1025): nxt <- values (first: ends without a slot get 0; later:
 *   they keep theirs); ends with nxt < 0 stepped through the surface: when `may_backstep`
 *   z0 -= back cur0 / z1 += back cur1, list <- their new points, *count = how many (else 0).
 * iso_raymarch_secant (:1114-1133) on n compacted rays: with f_mid = values at z_pred, move the
 *   bracket end of matching sign (f_mid > 0 -> lo, < 0 -> hi); then (also when f_mid is NULL: the
 *   first call) z_pred = -f_lo (z_hi - z_lo) / (f_hi - f_lo) + z_lo, pts_out = cam + z_pred d.  */
int iso_raymarch_settle(const float* cam, const float* dirs, int64_t n_rays, float* z, float* cur,
                        const float* nxt, uint8_t* live, float sdf_threshold, int check_order,
                        int step, int32_t* slot, float* list, int32_t* count, void* stream);
int iso_raymarch_overshoot(const float* cam, const float* dirs, int64_t n_rays, float* z,
                           const float* cur, float* nxt, const float* values, int first,
                           int may_backstep, float back, int32_t* slot, float* list,
                           int32_t* count, void* stream);
int iso_raymarch_secant(const float* cam, const float* dirs, int64_t n, float* f_lo, float* f_hi,
                        float* z_lo, float* z_hi, float* z_pred, const float* f_mid,
                        float* pts_out, void* stream);

/* Image values at projected points: get_tensor_values, DSS/utils/__init__.py:325-375
 * (= grid_sample(image (B,C,H,W), p, mode, padding_mode='reflection', align_corners=False),
 * squeezed and permuted).  p (B,n,2) in [-1,1] (x, y); out (B,n,C).
 * mode 0 bilinear, 1 nearest, 2 integer indexing trunc((p + 1)(size - 1)/2) (`grid_sample=False`,
 * :357-363; an index outside the image -- an IndexError in the reference -- gives NaN).          */
int iso_image_sample(const float* image, int batch, int channels, int height, int width,
                     const float* p, int64_t n, int mode, float* out, void* stream);

/* ------------------------------------------------------------------------
 * B. Fixed-radius nearest neighbours on a uniform grid
 *    replaces the third-party `frnn` / `prefix_sum` extensions the reference
 *    calls (lxxue/FRNN@eab337f, not vendored):
 *      frnn.frnn_grid_points  levelset_sampling.py:132,182,200
 *                             point_processing.py:74,84,145,179,253
 *                             rasterizer.py:371
 *      frnn.frnn_gather       levelset_sampling.py:213,268-271
 *      frnn._C.insert_points_cuda / counting_sort_cuda   rasterizer.py:909,921
 *      prefix_sum.prefix_sum_cuda                        rasterizer.py:915
 *
 *    Grid parameter block (f32), same layout the reference's kernels read
 *    (DSS/csrc/rasterize_points_backward.cu:10-28):
 *      3-D: [min_x,min_y,min_z, 1/cell, res_x,res_y,res_z, total]  (8 floats)
 *      2-D: [min_x,min_y,       1/cell, res_x,res_y,       total]  (6 floats)
 *    cell index = (x*res_y + y)*res_z + z   (2-D: x*res_y + y).
 * ---------------------------------------------------------------------- */
#define ISO_GRID3_PARAMS 8
#define ISO_GRID2_PARAMS 6
#define ISO_GRID_MAX_RES 256
/* upper bound of `total` for a grid built by iso_frnn_make_grid with max_res = ISO_GRID_MAX_RES */
#define ISO_GRID3_MAX_CELLS ((ISO_GRID_MAX_RES + 1) * (ISO_GRID_MAX_RES + 1) * (ISO_GRID_MAX_RES + 1))

/* Axis-aligned bounding box of each cloud: minmax (N,8) f32 =
 * [min_x,min_y,min_z,0, max_x,max_y,max_z,0] (zeros for an empty cloud).  Feeds the
 * search radius / kernel width of levelset_sampling.py:129-131 and :254-256 without
 * torch's dim-reductions or a host sync.                                         */
int iso_points_bbox(const float* points, const int64_t* lengths, int n_clouds,
                    int64_t p_stride, float* minmax, void* stream);

/* Device-side grid sizing for clouds `points` (N, P, 3) padded, lengths (N)
 * i64 (NULL = all P), radius (N) f32.  Writes params (N, 8).  Cell size is
 * chosen from point density (about 8 points per occupied cell on a surface)
 * but never finer than r/2 or (max extent)/max_res; the query walks Chebyshev
 * rings of cells so the result does not depend on the cell size.  No host
 * sync: the caller picks max_res (1..ISO_GRID_MAX_RES; 128 is plenty below ~250 k
 * points, 1 M points on a surface want 256) and allocates the grid arrays for
 * (max_res+1)^3 cells.                                                          */
int iso_frnn_make_grid(const float* points, const int64_t* lengths,
                       const float* radius, int n_clouds, int64_t p_stride,
                       int max_res, float* grid_params, void* stream);
/* The same with the density target spelled out: about `points_per_cell` points per occupied cell
 * on a surface (iso_frnn_make_grid = 8).  An exact K-nearest search (r = inf) finishes inside the
 * 3x3x3 cell neighbourhood -- the fast path of the query -- when the K-th neighbour is closer
 * than one cell; measured optimum points_per_cell ~ 0.75 K (K = 32, 150 k points on a surface:
 * 0.9 ms instead of 3.7 ms); results do not depend on the choice.                           */
int iso_frnn_make_grid_density(const float* points, const int64_t* lengths, const float* radius,
                               int n_clouds, int64_t p_stride, int max_res, float points_per_cell,
                               float* grid_params, void* stream);

/* frnn._C.insert_points_cuda: cell id and arrival slot of each point;
 * cnt (N,G) must be zero on entry.  dim = 2 or 3 (points have `dim` floats).  */
int iso_frnn_insert_points(const float* points, const int64_t* lengths,
                           const float* grid_params, int32_t* cnt,
                           int32_t* cell, int32_t* idx_in_cell, int n_clouds,
                           int64_t p_stride, int64_t g_stride, int dim,
                           void* stream);
/* prefix_sum.prefix_sum_cuda: exclusive scan of `n` i32 counts (in != out or
 * in == out).  `n` is read on the host; batch = independent rows.
 * workspace: iso_prefix_sum_workspace_bytes(n or g_stride, batch).           */
int64_t iso_prefix_sum_workspace_bytes(int64_t n, int batch);
int iso_prefix_sum(const int32_t* in, int32_t* out, int64_t n, int batch,
                   int64_t row_stride, void* workspace, int64_t workspace_bytes,
                   void* stream);
/* as iso_prefix_sum, but the row length is read ON DEVICE from
 * grid_params[total] and rows are scanned up to g_stride at most             */
int iso_frnn_scan_cells(const int32_t* cnt, int32_t* off,
                        const float* grid_params, int n_clouds,
                        int64_t g_stride, int dim, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* frnn._C.counting_sort_cuda: scatter points into cell order.
 * sorted_points (N,P,dim), sorted_idx (N,P) i32 = original index.            */
int iso_frnn_counting_sort(const float* points, const int64_t* lengths,
                           const int32_t* cell, const int32_t* idx_in_cell,
                           const int32_t* off, float* sorted_points,
                           int32_t* sorted_idx, int n_clouds, int64_t p_stride,
                           int64_t g_stride, int dim, void* stream);

/* Radius-K query (frnn.frnn_grid_points proper).  For every query point
 * q in points1 (N,P1,3): the K nearest points of cloud 2 with
 * d2 = (dx*dx + dy*dy) + dz*dz < r*r (f32, no FMA contraction), ascending by
 * (d2, original index); unused slots are -1 (idx) / -1.0 (dists).
 * idxs_out is i64 (pytorch3d convention, levelset_sampling.py:136).
 * nn_out (N,P1,K,3) may be NULL (return_nn=False); when given, points2
 * (N,P2,3, original order) must be given too.
 * points1 == NULL means "cloud 2 queried against itself": queries are then
 * processed in cell order (neighbouring lanes walk the same cells) and rows
 * are written at their original index.
 * sorted2 / sorted_idx2 / off come from the build calls above.
 * workspace (iso_frnn_query_workspace_bytes, 16-B aligned): list of the queries a single lane
 * could not finish within two rings of cells (a second kernel serves each of them with a whole
 * wave), and the per-call candidate records (x,y,z,index: one 16-B load per candidate).        */
int64_t iso_frnn_query_workspace_bytes(int n_clouds, int64_t p1_stride, int64_t p2_stride);
int iso_frnn_query(const float* points1, const int64_t* lengths1,
                   const float* points2, const float* sorted2,
                   const int32_t* sorted_idx2,
                   const int64_t* lengths2, const int32_t* off,
                   const float* grid_params, const float* radius, int K,
                   float* dists_out, int64_t* idxs_out, float* nn_out,
                   int n_clouds, int64_t p1_stride, int64_t p2_stride,
                   int64_t g_stride, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* The K nearest OTHER points of every point of cloud 2: iso_frnn_query with points1 == NULL (cloud 2 against itself,
 * rows written at their original index) and one difference: the candidate whose original index equals the query's own
 * row is passed over.  1 <= K <= 32, the same (d2, index) order, the same -1 / -1.0 padding, the same workspace
 * (iso_frnn_query_workspace_bytes(n_clouds, p2_stride, p2_stride)).  This is the "self plus K" search of the reference's
 * losses and filters (DSS/training/losses.py:169-180 asks pytorch3d for K = 33 and drops column 0) without the slot the
 * query's own point would take: on a cloud without duplicate points the result equals columns 1..K of a (K+1)-query.
 * With duplicates a (K+1)-query's column 0 may be the duplicate and not the point itself; here only the own row is left
 * out, so a duplicate is a neighbour at distance 0.                                                              */
int iso_frnn_query_others(const float* points2, const float* sorted2, const int32_t* sorted_idx2,
                          const int64_t* lengths2, const int32_t* off, const float* grid_params,
                          const float* radius, int K, float* dists_out, int64_t* idxs_out, float* nn_out,
                          int n_clouds, int64_t p2_stride, int64_t g_stride, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* frnn.frnn_gather: out[n,i,k,:] = x[n, idx[n,i,k], :], zeros where idx < 0.
 * x (N,P2,U) f32, idx (N,P1,K) i64, out (N,P1,K,U).                           */
int iso_frnn_gather(const float* x, const int64_t* idx, float* out,
                    int n_clouds, int64_t p1, int64_t p2, int K, int U,
                    void* stream);

/* ------------------------------------------------------------------------
 * C. Tangent-plane repulsion step
 *    replaces the body of UniformProjection.resample
 *    (DSS/models/levelset_sampling.py:268-284), single cloud:
 *      n_j = normalize(normals[j]) ; D = p_i - p_j ; w = exp(-|D|^2 * inv_sigma)
 *      Dt = D - (D.n_j) n_j ; move = (sum w + 1) * sum(w Dt) / sdeno(sum w)
 *      out_i = p_i + move_i
 *    Moves the n points [first_point, first_point+n) of `points` (rows 0..n-1 of idx and
 *    points_out belong to them; neighbour indices address the whole array) -- a rank of
 *    a sharded run passes its own slice, a single-GPU caller first_point = 0, n = P.
 *    idx: row i starts at idx + i*idx_row_stride (i64, K entries, -1 padding:
 *    weight 0 there) -- lets the caller pass the [:,1:] view of a (P,K+1)
 *    query result without copying.  inv_sigma (= P/diag, :256) is a DEVICE
 *    scalar so the bounding-box reduction needs no host sync.                 */
int iso_repulse(const float* points, const float* normals, const int64_t* idx,
                int64_t idx_row_stride, float* points_out, int64_t n,
                int64_t first_point, int K, const float* inv_sigma, void* stream);

/* UniformProjection.insert (DSS/models/levelset_sampling.py:172-233) on the device.
 * iso_insert_fathers: father[b][i] = 1 when the nearest of the n_refs (device int32, <= 64) selected reference
 *   points lies within the K = 1 query radius and 0 < d^2 < 4 spacing^2 (:200-206); params (device, 2 floats) =
 *   {(4 r)^2, 4 spacing^2}.
 * iso_insert_children: child = 2 father / 3 + neighbour / 3 over the LAST `patch` columns of knn_idx (:207-209),
 *   cloud b written from row out_first[b], fathers in ascending order (rank_inclusive = inclusive prefix sum of
 *   father over each cloud); neighbour index < 0 = the origin (what frnn_gather returns there).             */
int iso_insert_fathers(const float* points, const int64_t* lengths, int n_clouds, int64_t max_points,
                       const float* refs, const int32_t* n_refs, const float* params, uint8_t* father_out,
                       void* stream);
int iso_insert_children(const float* points, const int64_t* knn_idx, int n_clouds, int64_t max_points, int K,
                        int patch, const uint8_t* father, const int64_t* rank_inclusive, const int64_t* out_first,
                        float* children_out, void* stream);
/* Sparsest-edge candidates of point_processing.upsample
 * (DSS/utils/point_processing.py:326-339): per point p with neighbours nn_k (knn (n,K,3)):
 * mid_k = (nn_k + 2p)/3, spars_k = min_j |mid_k - nn_j|, sparsity = max_k spars_k,
 * candidate = mid_argmax (first maximum).  K <= 64.                               */
int iso_upsample_candidates(const float* points, const float* knn, int64_t n, int K,
                            float* sparsity_out, float* candidates_out, void* stream);

/* Edge-aware candidates of EdgeAwareProjection.upsample (DSS/models/levelset_sampling.py:609-628):
 * per point p (unit normal n) with neighbours nn_k (knn (n,K,3)) of unit normals u_k (knn_normals):
 * mid_k = (nn_k + 2p)/3, d_kj = mid_k - nn_j,
 * m_k = sqrt(max(|min_j (|d_kj| - sum_c (d_kj,c u_k,c)^2)|, 1e-17)), edge_k = (2 - n.u_k)^edge_sensitivity,
 * sparsity = max_k edge_k m_k, candidate = mid_argmax (first maximum).  K <= 64.             */
int iso_ear_candidates(const float* points, const float* normals, const float* knn,
                       const float* knn_normals, int64_t n, int K, float edge_sensitivity,
                       float* sparsity_out, float* candidates_out, void* stream);

/* Farthest-point sampling = torch_cluster.fps as wlop uses it
 * (DSS/utils/point_processing.py:473-499): per cloud n, out_idx[n, 0..n_samples[n]) =
 * start[n], then repeatedly the point farthest from the chosen set (squared f32 distances,
 * ties -> lowest index).  work: iso_farthest_point_sampling_work_floats(N, p_stride) f32 of
 * scratch.  out_idx rows are left untouched beyond n_samples[n] (n_samples[n] > length clamps
 * to the length, start[n] clamps into [0, length), an empty cloud's row is untouched).  Device
 * code keeps f32 denormals (the build sets no flush-to-zero flag), so the sequence is the IEEE
 * one at every scale.  Clouds of 4 096 .. 4 194 304 points (p_stride) run grid-wide (cooperative
 * launch, points held in registers: up to 2 097 152 points several samples per exchange, above
 * one), smaller ones in one workgroup per cloud with the points in registers, larger ones in
 * one workgroup walking memory; a device that refuses the cooperative launch runs one workgroup
 * per cloud, in registers up to 8 192 points; the sample sequence is the same.
 * iso_farthest_point_sampling_form reports the kernel a call with this p_stride takes: 0 the
 * memory-walking kernel, 100 + PPT registers of one workgroup, 200 + PPT grid-wide with several
 * samples per exchange, 300 + PPT grid-wide with one (PPT = points per thread), -1 for a stride
 * outside [1, 2^31).  check_device == 0 needs no GPU; != 0 also asks the current device whether
 * the cooperative grid can be co-resident and reports the one-workgroup form if not.
 * Test switches, read on every call: ISO_FPS_ONE_WORKGROUP (the memory-walking kernel for every
 * size) and ISO_FPS_NO_COOPERATIVE (behave as if the cooperative launch had been refused).  */
int64_t iso_farthest_point_sampling_work_floats(int n_clouds, int64_t p_stride);
int iso_farthest_point_sampling(const float* points, const int64_t* lengths,
                                const int64_t* n_samples, const int64_t* start, int n_clouds,
                                int64_t p_stride, int64_t out_stride, float* work,
                                int64_t* out_idx, void* stream);
int iso_farthest_point_sampling_form(int64_t p_stride, int check_device);

/* Local frames of a K-nearest neighbourhood = estimate_pointcloud_local_coord_frames
 * (DSS/utils/mathHelper.py:43-119): per valid row (b, i < lengths[b]) with neighbours
 * x_j = points[b, idx[b,i,j]] (idx (N,P,K) int64 from knn_points, the point itself included):
 * m = mean x_j, C = (1/K) sum (x_j - m)(x_j - m)^T, eigenpairs by cyclic Jacobi in f32,
 * eigenvalues clamped at >= 0 and ascending -> curvature_out (N,P,3); frames_out (N,P,3,3)
 * holds eigenvector c in column c (frames[..., :, 0] = the normal).  disambiguate != 0 applies
 * the reference's sign rule (:73-74, :105-113): with d_j = x_j - (p_i - mu_b), mu_b the mean of
 * cloud b's first lengths[b] rows, a column flips when #{<v, d_j> > 0} < K/2 (columns 0 and 2),
 * and column 1 = col0 x col2.  Rows i >= lengths[b] are zeroed; lengths NULL = max_points.
 * work: iso_pca_frames_work_bytes(N) of scratch (only read when disambiguate).  No atomics. */
int64_t iso_pca_frames_work_bytes(int n_clouds);
int iso_pca_frames(const float* points, const int64_t* lengths, const int64_t* idx, int n_clouds,
                   int64_t max_points, int K, int disambiguate, void* work, float* curvature_out,
                   float* frames_out, void* stream);

/* iso_pca_frames_backward: the gradient of iso_pca_frames w.r.t. the points = what autograd gives the
 * reference through DSS/utils/mathHelper.py:43-119 (kNN gather, torch_batch_svd's backward).  Held
 * constant: the index rows, the ascending order, the clamp at 0 and the two signs of the sign rule (the
 * cloud mean only enters a comparison and carries no gradient).  With curvature / frames the forward's own
 * outputs (l, V) and grad_curvature (N,P,3), grad_frames (N,P,3,3) the incoming gradients (either may be
 * NULL = zeros), per valid row i:
 *   disambiguate: gn = g_V[:,0] + z x g_V[:,1], gz = g_V[:,2] + g_V[:,1] x n, gv = (gn, 0, gz) against the
 *                 saved columns (n, n x z, z) -- G below is even in every column's sign; else gv = g_V;
 *   S_ab = (v_a.gv_b - v_b.gv_a) / (2 (l_b - l_a)), G_i = V (diag(g_l) + S) V^T;
 *   grad_points_out[t] = sum over the slots (i,j) with idx[i,j] = t, in ascending (i,j), of
 *                        (2/K) G_i (x_t - m_i),   m_i = the neighbourhood mean with the forward's bits.
 * Where the formula is undefined: a pair with |l_b - l_a| <= 2e-5 l_max gives S_ab = 0 (the tolerance the
 * forward's eigenvalues are judged by; below it the sign of the gap is not determined); a row with
 * l_max = 0 therefore gives G = 0; an eigenvalue that is 0 in `curvature` (clamped, or exactly 0) passes no
 * g_l; rows i >= lengths[b] give and receive nothing and their incoming gradients are never read (NaN
 * included).  Indices are clamped into the cloud as the forward clamps them.
 * Launches: the adjoint (one lane per row: G_i, m_i, the row's targets as int32), the counting sort of
 * the P*K slots by target (integer atomics, iso_prefix_sum), and the sum: a target in at most 64 slots
 * sorts its list and sums it in its own lane; longer lists take one wave each (sorted up to 1024 slots,
 * beyond that a strided scan of the slots) and one butterfly.  No float atomics: two runs give the same
 * bits.  Limit: N * P * K < 2^31 - 1.  work: iso_pca_frames_backward_work_bytes(N, P, K), 16-B aligned;
 * the size helper needs no GPU.                                                                        */
int64_t iso_pca_frames_backward_work_bytes(int n_clouds, int64_t max_points, int K);
int iso_pca_frames_backward(const float* points, const int64_t* lengths, const int64_t* idx,
                            int n_clouds, int64_t max_points, int K, int disambiguate,
                            const float* curvature, const float* frames,
                            const float* grad_curvature, const float* grad_frames, void* work,
                            int64_t work_bytes, float* grad_points_out, void* stream);

/* ------------------------------------------------------------------------
 * D. EWA surface splatting
 *    replaces SurfaceSplatting (DSS/core/rasterizer.py:103-661), the pybind module
 *    DSS._C (DSS/csrc/ext.cpp:5-18: splat_points, _splat_points_naive,
 *    _splat_points_occ_backward, _splat_points_occ_fast_cuda_backward,
 *    _backward_zbuf) and SurfaceSplattingRenderer.forward (DSS/core/renderer.py:36-82).
 *    Matrices are 4x4 row-major in pytorch3d's row-vector convention
 *    (p' = [p,1] @ M).  Packed clouds: cloud n owns rows
 *    [first_idx[n], first_idx[n]+num_pts[n]).
 * ---------------------------------------------------------------------- */

/* filter_renderable (rasterizer.py:184-254): flags (n_views, P) i32 = 1 when
 * znear <= z_view <= zfar and (backface_culling ? normal_view.z < 0 : 1).        */
int iso_splat_view_flags(const float* points, const float* normals, const float* views,
                         int32_t* flags, int64_t P, int n_views, float znear, float zfar,
                         int backface_culling, void* stream);
/* stable stream compaction of U-float rows: out[offsets[e]] = in[e % P] where
 * flags[e] != 0, e in [0,total) (offsets = exclusive scan of flags).           */
int iso_compact_rows(const float* in, const int32_t* flags, const int32_t* offsets,
                     float* out, int64_t P, int64_t total, int U, void* stream);
/* _compute_isotropic_Vrk (rasterizer.py:367-386): dists (N,p_stride,7) from the
 * K=7 self query -> h (packed) = clamp(0.5*max_{6 nn} d2, 5e-5, 0.01); clouds
 * with fewer than 7 points use d2 = 1e-3.  Row i of cloud n (i < num_pts[n]) is written to
 * h[first_idx[n] + i]; a rank that queried only a sub-range of each cloud passes the
 * sub-range in first_idx/num_pts and the true cloud sizes in cloud_num_pts (NULL = num_pts). */
int iso_splat_vrk_h(const float* dists, const int64_t* first_idx, const int64_t* num_pts,
                    const int64_t* cloud_num_pts, float* h, int n_clouds, int64_t p_stride,
                    void* stream);
/* _get_per_point_info + PointsRasterizer.transform (rasterizer.py:441-563,:618):
 * per packed point: NDC position (xy projected, z = view depth), ellipse (a,b,c),
 * cutoff, bbox radii, EWA normaliser.  views = world->view, projs = full
 * world->NDC, both (n_views,4,4).                                               */
int iso_splat_setup(const float* points, const float* normals, const float* h,
                    const int64_t* first_idx, const int64_t* num_pts, const float* views,
                    const float* projs, int n_views, int64_t max_pts, int image_size,
                    float sigma, float cutoff, float* ndc_out, float* ellipse_out,
                    float* cutoff_out, float* radii_out, float* scaler_out, void* stream);

/* _compute_global_Vrk (rasterizer.py:293-342), Vrk_invariant: ONE h per cloud.  dists (N,p_stride,7)
 * from the K=7 self query -> h[first_idx[n] + i] = clamp(mean, 5e-5, 1e-3) for every row of cloud n,
 * where mean is the reference's h_k.mean(dim=1) over the PADDED tensor of all clouds of ITS call:
 * sum over i < padded_len of 0.5*max_{6 nn} d2, with -0.5 for the rows past num_pts[n] (FRNN pads
 * distances with -1) and 0.5e-3 for every row of a cloud of fewer than 7 points, divided by
 * padded_len.  padded_len = the largest cloud's length over everything the reference would have
 * batched (>= p_stride; the caller may hand the clouds over in several calls with the same value).
 * num_pts[n] must be <= p_stride: rows of `dists` that do not exist count as padding.  Two launches:
 * per-slice sums in double (fixed order, no atomics), then finish + broadcast.
 * work: iso_splat_vrk_h_global_work_bytes(N) of scratch.                                   */
int64_t iso_splat_vrk_h_global_work_bytes(int n_clouds);
int iso_splat_vrk_h_global(const float* dists, const int64_t* first_idx, const int64_t* num_pts,
                           float* h, int n_clouds, int64_t p_stride, int64_t padded_len, void* work,
                           void* stream);
/* The tangent frame the isotropic set-up (iso_splat_setup / iso_splat_front) derives from a normal:
 * u = normalize(n x (n + e)), v = normalize(n x u), e = the axis least aligned with n.  n rows of
 * normals -> u_out, v_out (n,3).  For tests and tools: iso_splat_setup_vrk fed (n, u, v) and
 * curvature (., h, h) gives iso_splat_setup's bits.                                         */
int iso_splat_tangent_frame(const float* normals, int64_t n, float* u_out, float* v_out, void* stream);
/* _get_per_point_info with an explicit local frame (_compute_anisotropic_Vrk, rasterizer.py:257-291
 * + :417-424): as iso_splat_setup, but the splat's plane and variances come from frames (P,3,3)
 * packed (eigenvector c in column c) and curvature (P,3) packed, ascending, as iso_pca_frames
 * writes them: u = column 1, v = column 2, Vrk = curvature[1] u u^T + curvature[2] v v^T (no clamp).
 * Every output is invariant under a sign flip of u or v.  A row with curvature[1] == curvature[2]
 * takes iso_splat_setup's factored arithmetic.                                             */
int iso_splat_setup_vrk(const float* points, const float* frames, const float* curvature,
                        const int64_t* first_idx, const int64_t* num_pts, const float* views,
                        const float* projs, int n_views, int64_t max_pts, int image_size,
                        float sigma, float cutoff, float* ndc_out, float* ellipse_out,
                        float* cutoff_out, float* radii_out, float* scaler_out, void* stream);
/* The same, fused with estimate_pointcloud_local_coord_frames(neighborhood_size=8,
 * disambiguate_directions=False) (mathHelper.py:43-119): knn_idx (n_views,p_stride,8) int64 holds,
 * for row i of view cloud n, the 8 nearest rows of THAT cloud (the row itself included, indices
 * local to the cloud: knn_points on the padded view clouds); the frame is solved in registers by
 * the device code of iso_pca_frames and never written.  Bit-identical to iso_pca_frames(K=8,
 * disambiguate=0) + iso_splat_setup_vrk.  Every cloud must hold more than 8 points.          */
int iso_splat_setup_aniso(const float* points, const int64_t* knn_idx, int64_t p_stride,
                          const int64_t* first_idx, const int64_t* num_pts, const float* views,
                          const float* projs, int n_views, int image_size, float sigma,
                          float cutoff, float* ndc_out, float* ellipse_out, float* cutoff_out,
                          float* radii_out, float* scaler_out, void* stream);

/* Forward rasterisation = _C.splat_points (rasterize_points.h:461-525).
 * Two calls around one caller-side read of the pair count:
 *   iso_splat_bin_count : tile_cnt (n_clouds*T*T, zero on entry) += splats per
 *                         16x16 tile (T = iso_splat_tiles_per_side(S));
 *   caller: tile_off = exclusive scan (iso_prefix_sum), total = off[last]+cnt[last],
 *           allocate `pairs` (i32, >= total), zero tile_cursor (n_clouds*T*T i32) and
 *           overflow_flag; tile_off needs n_clouds*T*T + 1 entries (the last = total);
 *   iso_splat_forward   : fill + raster (tile_cursor holds the fill cursors first and is then
 *                         overwritten with the heaviest-first tile order the raster walks).  Per pixel the points_per_pixel (<= 150; above 32 a slow kernel that keeps the lists in the outputs)
 *                         smallest (z, idx) hits, entries with z - z0 >
 *                         depth_merging_thres reset to -1, occupancy = any hit.
 * Outputs as the reference: idx i32, zbuf/qvalue f32 (N,S,S,K), occ f32 (N,S,S),
 * image flipped in both axes (+X left, +Y up).  *overflow_flag != 0 afterwards
 * means pair_capacity was too small (result incomplete).
 * workspace (optional, NULL = none): iso_splat_forward_workspace_bytes(tiles of the band, K); with it
 * the tiles that hold many times the mean number of candidates (silhouettes) are rasterised in slices
 * by several workgroups and merged -- same result, the longest work item is a slice.
 * Non-square images (beyond the reference, whose rasteriser is square-only, rasterizer.py:52): image_size
 * = rows H, image_width = columns W (<= 0: W = H); outputs (N,H,W,K).  NDC follows pytorch3d's non-square
 * convention: the shorter side spans [-1,1], the longer [-e,e], e = longer / shorter -- square pixels of
 * 2 / min(H,W); the per-point set-up (iso_splat_setup / iso_splat_front) takes image_size = min(H,W).
 * T = iso_splat_tiles_per_side(H) tile rows, iso_splat_tiles_per_side(W) tile columns.
 * [tile_row_begin, tile_row_end) restricts both calls to a band of tile rows (in NDC pixel
 * order, i.e. before the flip): a rank of a sharded run rasterises only its band and leaves
 * the other pixels of the output tensors untouched; pass 0, T for the whole image.          */
int iso_splat_tiles_per_side(int image_size);
int iso_splat_bin_count(const float* points, const float* radii, const int64_t* first_idx,
                        const int64_t* num_pts, int n_clouds, int64_t max_pts, int image_size,
                        int image_width, int tile_row_begin, int tile_row_end, int32_t* tile_cnt,
                        void* stream);
/* Offsets of the tile lists from the counts of iso_splat_bin_count in ONE launch: tile_off = exclusive scan of
 * tile_cnt[0..n) (n = views x tiles + 1; same result as iso_prefix_sum), tile_cursor[0..n) = 0 (the fill cursors and,
 * in the last word, the overflow flag iso_splat_forward expects cleared), and tile_cnt is cleared as it is read, so
 * a caller that keeps the counter array never clears it again.                                        */
int iso_splat_tile_offsets(int32_t* tile_cnt, int32_t* tile_off, int32_t* tile_cursor, int64_t n, void* stream);
int iso_splat_forward(const float* points, const float* ellipse, const float* cutoff,
                      const float* radii, const int64_t* first_idx, const int64_t* num_pts,
                      int n_clouds, int64_t max_pts, float depth_merging_thres, int image_size,
                      int image_width, int points_per_pixel, int tile_row_begin, int tile_row_end,
                      int32_t* tile_cursor, const int32_t* tile_off,
                      int32_t* pairs, int64_t pair_capacity, int32_t* overflow_flag,
                      int32_t* idx_out, float* zbuf_out, float* qvalue_out, float* occ_out,
                      void* workspace, int64_t workspace_bytes, void* stream);
int64_t iso_splat_forward_workspace_bytes(int64_t n_tiles, int points_per_pixel);
/* iso_splat_forward and iso_splat_composite (below) in one pass: image_out (N,S,S,channels+1) is
 * composited from the pixels' K-best lists while they are in registers -- same arithmetic and order,
 * the (N,S,S,K) lists are written as before (the backward needs them) but not read again.       */
int iso_splat_render(const float* points, const float* ellipse, const float* cutoff,
                     const float* radii, const int64_t* first_idx, const int64_t* num_pts,
                     int n_clouds, int64_t max_pts, float depth_merging_thres, int image_size,
                     int image_width, int points_per_pixel, int tile_row_begin, int tile_row_end,
                     int32_t* tile_cursor, const int32_t* tile_off,
                     int32_t* pairs, int64_t pair_capacity, int32_t* overflow_flag,
                     int32_t* idx_out, float* zbuf_out, float* qvalue_out, float* occ_out,
                     void* workspace, int64_t workspace_bytes, const float* scaler,
                     const float* features, int channels, int norm_weighted, float eps,
                     float* image_out, void* stream);

/* iso_splat_render that also leaves the visible flags of the backward pass (iso_splat_mark_visible: rasterizer.py:850-853
 * of the reference marks the points listed in the pixels' lists) while it writes the lists: visible_out (P,) uint8, ZERO
 * on entry over the rows of the clouds (iso_splat_front_rows clears them), NULL = iso_splat_render.               */
int iso_splat_render_visible(const float* points, const float* ellipse, const float* cutoff,
                             const float* radii, const int64_t* first_idx, const int64_t* num_pts,
                             int n_clouds, int64_t max_pts, float depth_merging_thres, int image_size,
                             int image_width, int points_per_pixel, int tile_row_begin, int tile_row_end,
                             int32_t* tile_cursor, const int32_t* tile_off,
                             int32_t* pairs, int64_t pair_capacity, int32_t* overflow_flag,
                             int32_t* idx_out, float* zbuf_out, float* qvalue_out, float* occ_out,
                             void* workspace, int64_t workspace_bytes, const float* scaler,
                             const float* features, int channels, int norm_weighted, float eps,
                             float* image_out, uint8_t* visible_out, void* stream);

/* The reference's two-stage raster interface, DSS._C._rasterize_coarse / _rasterize_fine (DSS/csrc/ext.cpp:11-12;
 * dispatchers rasterize_points.h:167,257; kernels rasterize_points.cu:293-441, :503-596).  No Python caller in the
 * reference (splat_points runs both internally); here they are a compatibility surface beside iso_splat_forward, whose
 * own binning is the tile lists of iso_splat_bin_count.
 *   coarse: bin_points_out (N, B, B, M) int32, B = 1 + (image_size - 1) / bin_size: bin (by, bx) lists the packed
 *           indices of its cloud's points with z >= 0 whose box [p - r, p + r] overlaps the bin (extent = PixToNdc of
 *           its first / last pixel -+ half a pixel, non-strict), ascending (the reference: arrival order of its atomics
 *           on the GPU, ascending on the CPU), -1 behind them; *overflow_out is set to 1 when a bin had more than M
 *           (cut at M; never cleared here).
 *   fine:   per pixel the K front-most hits among the entries of its bin (negative entries skipped), tests and outputs
 *           of iso_splat_forward: fine(coarse(x)) == iso_splat_forward(x) bit for bit when no bin overflowed.  K <= 150 (above 32: the
 *           lists are kept in the output arrays, as in iso_splat_forward). */
int iso_rasterize_coarse(const float* points, const float* radii, const int64_t* first_idx, const int64_t* num_pts,
                         int n_clouds, int image_size, int bin_size, int max_points_per_bin, int32_t* bin_points_out,
                         int32_t* overflow_out, void* stream);
int iso_rasterize_fine(const float* points, const float* ellipse, const float* cutoff, const float* radii,
                       int64_t n_points, const int32_t* bin_points, int n_clouds, int max_points_per_bin,
                       float depth_merging_thres, int image_size, int bin_size, int points_per_pixel,
                       int32_t* idx_out, float* zbuf_out, float* qvalue_out, float* occ_out, void* stream);

/* DSS/utils/__init__.py:172-185 (gather_with_neg_idx) for one float per point, as SurfaceSplatting.forward uses it for
 * the fragments' scaler (rasterizer.py:635-637): out[i] = idx[i] >= 0 ? values[idx[i]] : 0, i < n.  idx and out must be
 * 16-byte aligned (they are read and written four entries at a time): ISO_ERR_INVALID otherwise.  The Python
 * gather_with_neg_idx takes its torch route for an index view that is not.                                            */
int iso_gather_neg_idx(const float* values, const int32_t* idx, int64_t n, float* out, void* stream);

/* renderer.py:53-78: w = exp(-0.5 q) * scaler[idx] (0 where idx < 0);
 * image[..., c] = sum_k w f / max(sum_k w, eps) (norm_weighted) or sum_k w f;
 * image[..., channels] = occupancy.  frag_scaler_out (n_pixels,K) may be NULL.
 * Which kernel runs: points_per_pixel 8 or 4 with channels <= 3 and idx, qvalue and frag_scaler_out (NULL counts) all
 * 16-byte aligned take a form that holds the pixel's list in registers; every other K, channel count or alignment the
 * generic loop.  All forms, and the raster's fused epilogue (iso_splat_render), do the same operations in the same
 * order: bit-identical images (tests/test_composite_gpu.py).  channels <= 8 here and in the backward
 * (ISO_ERR_UNSUPPORTED above); the Python composite() runs wider features in chunks of 8 channels.  */
int iso_splat_composite(const int32_t* idx, const float* qvalue, const float* occ,
                        const float* scaler, const float* features, int64_t n_pixels,
                        int points_per_pixel, int channels, int norm_weighted, float eps,
                        float* frag_scaler_out, float* image_out, void* stream);

/* Backward = EllipticalRasterizer.backward, default fast path
 * (rasterizer.py:841-968 + rasterize_points_backward.cu:85-178 +
 * rasterize_points.cu:823-846), point-major and atomic-free:
 *   iso_splat_mark_visible: visible[p] = 1 for points listed in pixels whose first
 *                           slot is filled (visible zeroed by the caller);
 *   iso_splat_backward    : grad_points (P,3): xy = sum over pixels within
 *                           search_radius[n] of grad_occ * d/sdeno(|d|^2,1e-10)
 *                           (visible points; grad>0 pixels outside the splat rect
 *                           skipped), z = sum of grad_zbuf over the slots that list
 *                           the point.  No float atomics: a point's xy terms are added in image
 *                           order by eight lanes whose partial sums meet in a fixed tree, the z sum
 *                           is a pixel-major scatter in 64-bit fixed point (integer atomics, exactly
 *                           rounded) -> bit-stable.
 *                           total_points = rows of `points` (sizes the heavy-point list).
 *                           workspace: iso_splat_backward_workspace_bytes, 16-byte aligned (it starts
 *                           with 64-bit pixel masks of the gradient image).
 * grad_zbuf/idx may be NULL (no z gradient); visible may be NULL (= all).
 * rect_mode = 1 switches the xy support to the slow reference kernel's rectangle
 * |d| <= radii * radii_s (_C._splat_points_occ_backward, rasterize_points.cu:673-760);
 * search_radius is then unused.                                                  */
/* Backward of iso_splat_composite (renderer.py:53-78 composites through pytorch3d's differentiable
 * compositors): grad_image (n_pixels, channels + 1) -> grad_features (P, channels) and grad_scaler (P)
 * ACCUMULATED into the caller's zero-initialised buffers (float atomics), grad_qvalue (n_pixels, K)
 * and grad_occ (n_pixels) written; any output pointer may be NULL.                               */
int iso_splat_composite_backward(const int32_t* idx, const float* qvalue, const float* scaler,
                                 const float* features, const float* grad_image, int64_t n_pixels,
                                 int points_per_pixel, int channels, int norm_weighted, float eps,
                                 float* grad_features, float* grad_qvalue, float* grad_scaler,
                                 float* grad_occ, void* stream);
int iso_splat_mark_visible(const int32_t* idx, int64_t n_pixels, int points_per_pixel,
                           uint8_t* visible, void* stream);
/* search_radius_out[n] = lower-median(radii of the visible points of cloud n, both columns
 * flattened) * radii_s  (rasterizer.py:884, torch.median semantics), 0 for a cloud without
 * visible points.  Exact: radix select on the f32 bit patterns, three histogram passes (11 + 11 + 10 bits) and
 * a final pass.  The workspace holds the histograms: it must be ZERO on entry and is left zero on exit, so a
 * caller that keeps one workspace clears it once (hipMemset) and never again.                        */
int64_t iso_splat_median_radius_workspace_bytes(int n_clouds);
int iso_splat_median_radius(const float* radii, const uint8_t* visible, const int64_t* first_idx,
                            const int64_t* num_pts, int n_clouds, int64_t max_pts, float radii_s,
                            void* workspace, int64_t workspace_bytes, float* search_radius_out,
                            void* stream);
int64_t iso_splat_backward_workspace_bytes(int n_clouds, int image_size, int image_width,
                                           int64_t total_points);
int iso_splat_backward(const float* points, const float* radii, const uint8_t* visible,
                       const float* search_radius, const int64_t* first_idx,
                       const int64_t* num_pts, int n_clouds, int64_t max_pts,
                       const float* grad_occ, const int32_t* idx, const float* grad_zbuf,
                       int image_size, int image_width, int points_per_pixel, int rect_mode, float radii_s,
                       int64_t total_points, void* workspace, int64_t workspace_bytes,
                       float* grad_points, void* stream);
/* _C._backward_zbuf alone (rasterize_points.cu:823-846): z_grad[idx] += grad_zbuf
 * by atomic scatter, accumulating into the caller's (P) buffer.                 */
int iso_splat_zbuf_backward(const int32_t* idx, const float* grad_zbuf, int64_t n_pixels,
                            int points_per_pixel, float* z_grad, void* stream);

/* ------------------------------------------------------------------------
 * E. Brick grid + fused neighbour kernels (the hot path of the iso-point cycle)
 *
 *    The stand-alone FRNN entry points of section B stay the general API.  The cycle itself
 *    (UniformProjection.resample, levelset_sampling.py:239-288, and the K = 7 bandwidth query of
 *    SurfaceSplatting._get_per_point_info, rasterizer.py:367-386) runs on a two-level grid:
 *    coarse BRICKS of 4x4x4 fine cells in global memory (x-major brick id, so a range of brick
 *    ids is an x-slab of space -- the unit the multi-GPU path shards by), fine cells only in LDS:
 *    a workgroup stages its brick plus a one-cell halo, counting-sorted by fine cell, and every
 *    query of the brick walks its 3x3x3 fine cells there.  Exact results (K nearest within r,
 *    ties to the lower id): a query whose K-th distance is not covered by the staged block is
 *    finished by a tail kernel that walks rings of bricks.
 *
 *    One workspace (iso_bricks_workspace_bytes(n_max), 256-B aligned) holds the grid; n_max =
 *    n_own + import_max must be the same in every call on that workspace.
 *
 *    iso_bricks_build: bbox = [min xyz, 0, max xyz, 0] on the device (iso_points_bbox layout; N
 *    ranks reduce it first so that every rank derives the same grid), n_total = points of the
 *    WHOLE cloud.  radius > 0: fixed search radius; radius <= 0: r = sqrt(|bbox diag| / n_total)
 *    * knn_k (levelset_sampling.py:129-131).  Fine cell = cell_scale * sqrt(diag / n_total),
 *    clamped to [extent / (4 (cap-1)), 1.002 r].  Own points get ids id_base + i; the optional
 *    imported records (halo cells of other ranks: rec0 = x,y,z,id-bits, rec1 = nx,ny,nz,payload,
 *    count on the device) are searched but never queried.  payload: one int per own point
 *    carried to the kernels (the view mask for iso_splat_h_fused), or NULL.
 * ---------------------------------------------------------------------- */
int64_t iso_bricks_workspace_bytes(int64_t n_max);
/* Once per workspace, before its first build: zeroes the brick counters and the counter block.  Every build leaves
 * the brick counters zeroed again (the offsets pass clears what it has read), so no build starts with a clearing
 * pass.  The counter block (576 ints at byte 256 of the workspace; behind it, also at a fixed offset, the 2048 zero-on-entry
 * chunk totals of the brick scan): [0..15] counters of the current grid (slots as
 * documented below), [16..31] "sticky" sums of the counters of all earlier grids on this workspace -- a header write
 * adds what it resets -- so that a caller can check the overflow / certification counters of a whole cycle of several
 * grids with one read afterwards.                                                                    */
int iso_bricks_workspace_init(void* workspace, int64_t n_max, void* stream);
/* Diagnostic, synchronises `stream`: ISO_ERR_INVALID when iso_bricks_workspace_init never ran on this workspace (it
 * leaves a mark in the counter block).  A build on such a workspace counts into whatever the memory held and gives a
 * wrong grid with no other sign; the builds themselves cannot check (the mark lives on the device).  Also refuses a
 * workspace whose arrival words or scan totals are not zero (an aborted build left them set: every later build on it
 * would compute wrong offsets).                                                                                  */
int iso_bricks_workspace_check(const void* workspace, int64_t n_max, void* stream);
/* iso_bricks_build for ONE rank that holds the whole cloud (n_total = n, id_base = 0, no imports): the bounding box
 * is taken by the build itself -- no iso_points_bbox pass, no 8-float round trip (six launches per grid instead of
 * twelve).  Same grid, same results as iso_points_bbox + iso_bricks_build.                          */
int iso_bricks_build_whole(const float* points, const float* normals, const int32_t* payload, int64_t n,
                           float radius, int knn_k, float cell_scale, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* iso_bricks_build_whole without its box pass: the bounding box of `points` is the workspace's PENDING BOX, left there by
 * the launch that wrote the points (iso_project_*_follow).  follow_host != NULL with views: the per-tile counts that launch
 * left in follow_host->front_ws are scanned on the side (one workgroup more in the count launch): front_ws, first_idx_out,
 * num_pts_out, view_total_out as iso_splat_view_mask_scan leaves them.                                  */
int iso_bricks_build_pending(const float* points, const float* normals, const int32_t* payload, int64_t n,
                             float radius, int knn_k, float cell_scale, void* workspace,
                             int64_t workspace_bytes, const iso_follow* follow_host, void* stream);
/* the pending box as 8 floats (iso_points_bbox layout), cleared afterwards: N ranks all-gather it for iso_bricks_params */
int iso_bricks_box_take(void* workspace, int64_t n_max, float* box_out, void* stream);
int iso_bricks_build(const float* points, const float* normals, const int32_t* payload,
                     int64_t n_own, int64_t id_base, const float* import_rec0,
                     const float* import_rec1, const int32_t* import_count, int64_t import_max,
                     const float* bbox, int64_t n_total, float radius, int knn_k,
                     float cell_scale, void* workspace, int64_t workspace_bytes, void* stream);
/* N ranks, one x-slab of the cloud each: every rank derives the SAME grid from the
 * reduced bounding box (iso_bricks_params), exports the points other ranks' queries can reach
 * (iso_halo_export: fine x-cell within one cell of another rank's local x-range; rank_boxes =
 * (world, 8) floats, every rank's local iso_points_bbox), the export buffers are all-gathered
 * (one RCCL all-gather of `export_buf`: float4[2][capacity + 1], word 0 = record count), and each
 * rank keeps what its own queries can reach (iso_halo_import) as the imported records of
 * iso_bricks_build (bbox = NULL: header already written).  halo_cells: width of the exchanged band in
 * fine cells (>= 1; the fused kernels certify their results within one cell, the tail kernels -- a query
 * whose K-th neighbour lies farther -- check their search ball against the imported band and count the
 * queries that left it).  The grid's counters: slot 4 an exporter ran out of capacity, slot 5 the import
 * buffer did, slot 6 tail queries that needed more than the imported band.                       */
/* boxes: n_boxes rows of 8 floats (iso_points_bbox layout: every rank's local box as all-gathered); the header is
 * written for their union.                                                                          */
int iso_bricks_params(const float* boxes, int n_boxes, int64_t n_total, int64_t n_own, int64_t id_base, float radius,
                      int knn_k, float cell_scale, void* workspace, int64_t n_max, void* stream);
int iso_halo_export(void* workspace, const float* points, const float* normals, const int32_t* payload,
                    int64_t n_own, const float* rank_boxes, int world, int rank, int halo_cells,
                    float* export_buf, int64_t capacity, void* stream);
int iso_halo_import(void* workspace, int64_t n_max, const float* gathered, const float* rank_boxes, int world,
                    int rank, int halo_cells, int64_t capacity, float* import_rec0, float* import_rec1,
                    int32_t* import_count, int64_t import_capacity, void* stream);
/* One resample move of every own point: K+1 = k_plus_one self-inclusive FRNN query (radius of
 * the build), column 0 dropped, tangent-plane repulsion with inv_sigma = n_total / diag
 * (levelset_sampling.py:254-284; same arithmetic as iso_frnn_query + iso_repulse).  `points`
 * = the own points the grid was built from.  idx_out (n_own, K) int64 / d2_out (n_own, K)
 * optional: the neighbour lists (UniformProjection._knn_idx / _knn_dists).            */
int iso_resample_fused(void* workspace, int64_t n_max, const float* points, int64_t n_own,
                       int k_plus_one, float* points_out, int64_t* idx_out, float* d2_out,
                       void* stream);
/* mask_out[i] bit v = point i is renderable in view v (z range + backface culling,
 * rasterizer.py:184-254; = iso_splat_view_flags for up to 8 views at once);
 * view_count_out[0..7] = points per view.                                            */
int iso_splat_view_mask(const float* points, const float* normals, const float* views, int n_views,
                        int64_t n, float znear, float zfar, int backface_culling,
                        int32_t* mask_out, int32_t* view_count_out, void* stream);
/* h_out[v * n_own + i] = clamp(max d2 of the 6 nearest OTHER points renderable in view v within
 * the build radius / 2, 5e-5, 0.01) for every view v in which own point i is renderable
 * (rasterizer.py:367-386; = iso_frnn_query K = 7 on each filtered view cloud + iso_splat_vrk_h),
 * all views in one pass over the grid (payload = view mask).  view_total[v] = points of the
 * whole cloud renderable in view v (< 7: the reference's 1e-3 branch).                */
int iso_splat_h_fused(void* workspace, int64_t n_max, const float* points, const int32_t* mask,
                      int64_t n_own, const int32_t* view_total, int n_views, float* h_out,
                      void* stream);
/* Front end of the splat for ONE cloud seen by up to 8 cameras, on the unfiltered cloud and without a
 * host read: mask (iso_splat_view_mask) + h (iso_splat_h_fused) -> the packed per-view arrays that
 * _C.splat_points takes (SurfaceSplatting.forward, rasterizer.py:597-661: filter, extend to the
 * cameras, _get_per_point_info, transform).  Packed order = view-major, points ascending (the
 * reference's); first_idx_out / num_pts_out (n_views) int64 and view_total_out (8) int32 are written
 * on the device; the per-point outputs must hold n_views * n_points rows (upper bound), rows beyond
 * first[n_views-1] + num[n_views-1] stay untouched.  features (n_points, channels) -> features_out
 * packed, or features_from_normals = 1: 0.5 (normalize(n) + 1) (3 channels); src_out: original point of
 * every packed row (scatter of the row gradients back to the cloud).  Same arithmetic as
 * iso_splat_view_flags + iso_compact_rows + iso_splat_setup.                                     */
int64_t iso_splat_front_workspace_bytes(int64_t n_points);
int iso_splat_front(const float* points, const float* normals, const float* features, int channels,
                    int features_from_normals, const int32_t* mask, const float* h, int64_t n_points,
                    const float* views, const float* projs, int n_views, int image_size, float sigma,
                    float cutoff, void* workspace, int64_t workspace_bytes, int64_t* first_idx_out,
                    int64_t* num_pts_out, int32_t* view_total_out, float* ndc_out, float* ellipse_out,
                    float* cutoff_out, float* radii_out, float* scaler_out, float* features_out,
                    int32_t* src_out, void* stream);
/* The same front end with two launches fewer and the view totals known BEFORE the bandwidth pass needs them:
 * iso_splat_view_mask_scan = renderable mask (iso_splat_view_mask's rule) + per-chunk counts + their scan: mask_out,
 * first_idx_out / num_pts_out (n_views int64) and view_total_out (8 int32) are final, the workspace
 * (iso_splat_front_workspace_bytes) holds the scanned chunk table; iso_splat_front_rows = the compaction + set-up pass
 * of iso_splat_front alone, on that workspace / mask / first_idx.                                     */
int iso_splat_view_mask_scan(const float* points, const float* normals, const float* views, int n_views,
                             int64_t n_points, float znear, float zfar, int backface_culling, int32_t* mask_out,
                             void* workspace, int64_t workspace_bytes, int64_t* first_idx_out, int64_t* num_pts_out,
                             int32_t* view_total_out, void* stream);
int iso_splat_front_rows(const float* points, const float* normals, const float* features, int channels,
                         int features_from_normals, const int32_t* mask, const float* h, int64_t n_points,
                         const float* views, const float* projs, int n_views, int image_size, float sigma,
                         float cutoff, const void* workspace, int64_t workspace_bytes, const int64_t* first_idx,
                         float* ndc_out, float* ellipse_out, float* cutoff_out, float* radii_out,
                         float* scaler_out, float* features_out, int32_t* src_out,
                         uint8_t* visible_zero_out /* (rows) or NULL: the rows' "visible" flags of the backward pass
                                                      (iso_splat_mark_visible), cleared here instead of by a fill */,
                         int64_t row_capacity /* rows the output arrays hold; <= 0: num_points.sum() rows, whatever that is */,
                         int32_t* overflow_out /* set to 1 when rows were dropped at row_capacity (never cleared here), or NULL */,
                         void* stream);
/* Gradient of the packed NDC rows of iso_splat_front w.r.t. the WORLD points (the part of the reference's
 * backward that autograd runs through cameras.transform_points in SurfaceSplatting.transform,
 * rasterizer.py:565-582,618: per-point set-up is under no_grad :608-610, so d(ndc)/d(point) is all there is).
 * grad_ndc (rows,3) -> grad_points (n_points,3), summed over the views a point is rendered in (ascending view
 * order, deterministic); mask / src / first_idx / num_points as written by iso_splat_view_mask / iso_splat_front. */
int iso_splat_points_backward(const float* points, int64_t n_points, const float* views, const float* projs,
                              int n_views, const int32_t* mask, const int32_t* src, const int64_t* first_idx,
                              const int64_t* num_points, const float* grad_ndc, float* grad_points, void* stream);
/* The z gradient of iso_splat_backward in pieces, for N ranks that each own a band of tile rows:
 * zscale (2 ints: bits of max |grad_zbuf|, exponent) <- iso_splat_z_absmax over the rank's pixels, MAX-
 * reduced over the ranks (word 0); iso_splat_z_scatter derives the exponent and adds the rank's pixels
 * into the zero-initialised 64-bit accumulators acc (total rows); acc is SUM-reduced over the ranks;
 * iso_splat_z_finish converts rows [row0, row0 + n_rows) into grad_points[:, 2].  Exactly rounded and
 * order independent like the single-GPU path (ZbufBackwardKernel, rasterize_points.cu:823-846).     */
int iso_splat_z_absmax(const float* grad_zbuf, int64_t n, int32_t* zscale, void* stream);
int iso_splat_z_scatter(const int32_t* idx, const float* grad_zbuf, int64_t n_pixels, int points_per_pixel,
                        int64_t pixels_per_view, int32_t* zscale, int64_t* acc, void* stream);
int iso_splat_z_finish(const int64_t* acc, const int32_t* zscale, int64_t row0, int64_t n_rows,
                       float* grad_points, void* stream);
/* The same for the band of EVERY view in one call each (a rank's band = rows [y0, y1) of all n_views images of the
 * (N,H,W,K) arrays; idx / grad_zbuf point at the band's first pixel of view 0, view_pixels = H * W, band_pixels =
 * (y1 - y0) * W): iso_splat_band_marks = iso_splat_mark_visible + iso_splat_z_absmax (zscale zeroed first) over
 * the n_views slices, iso_splat_band_z_scatter = iso_splat_z_scatter over them (pixels_per_view = view_pixels).
 * Two launches per call instead of two per view -- a rank's share of a cycle is a chain of small kernels.   */
int iso_splat_band_marks(const int32_t* idx, const float* grad_zbuf, int n_views, int64_t view_pixels,
                         int64_t band_pixels, int points_per_pixel, uint8_t* visible, int32_t* zscale, void* stream);
int iso_splat_band_z_scatter(const int32_t* idx, const float* grad_zbuf, int n_views, int64_t view_pixels,
                             int64_t band_pixels, int points_per_pixel, int32_t* zscale, int64_t* acc, void* stream);
/* N ranks: the packed per-view arrays of the WHOLE cloud (view-major, then rank, then the rank's own
 * order = the single-GPU order when the ranks hold consecutive ranges of the cloud) from the
 * all-gathered per-rank outputs of iso_splat_front.  gathered: world blocks of 12 * capacity floats
 * (ndc 3, ellipse 3, radii 2, scaler 1, features 3 -- the front end's outputs laid out in one
 * buffer); counts (world, 8) int32: the ranks' view_total_out.  own_first / own_num: this rank's
 * rows inside the global layout.                                                              */
int iso_splat_repack(const float* gathered, int64_t capacity, int world, int rank, int n_views,
                     const int32_t* counts, float cutoff, int64_t max_rows, float* ndc_out,
                     float* ellipse_out, float* cutoff_out, float* radii_out, float* scaler_out,
                     float* features_out, int64_t* first_idx_out, int64_t* num_pts_out,
                     int64_t* own_first_out, int64_t* own_num_out, void* stream);

/* ----------------------------------------------------------------------
 * F. N ranks, splat stage: the fragment-side exchange (csrc/band.hip; SURVEY 8(e) -- the reference has no
 *    distributed layer; the cell order it shards by is that of DSS/csrc/rasterize_points_backward.cu:119).
 *
 *    Every rank runs the front end on its own points and rasterises a BAND of 16-pixel tile rows of every view
 *    (the balanced split of the tile rows over the ranks).  A packed row is needed by exactly the bands its
 *    bounding box touches (the binning pass's test), so it is sent to those ranks only, in ONE all-to-all with equal
 *    splits: `send` = world segments of iso_splat_band_segment_floats(cap_pair) floats, each a 16-int header
 *    ([0..7] records per view, [8] records wanted) and cap_pair records of 13 floats (ndc 3, ellipse 3, radii 2,
 *    scaler 1, features 3, the row's GLOBAL id: its position in the single-GPU packed layout).  Rows keep their
 *    order inside a segment.  iso_splat_band_import lays the received segments out view-major and, inside a view, by
 *    source rank: ascending global id, so the (z, id) tie rule of the rasteriser picks what the single-GPU run picks;
 *    iso_splat_band_remap turns the band's per-pixel local row ids into the global ones (= the single-GPU lists).
 *    Backward: the band's per-record results (64-bit fixed-point z sum, visible flag) go back into the slots the
 *    records came in (iso_splat_band_return: world segments of cap_pair x 2 int64), the reverse all-to-all returns
 *    them, iso_splat_band_merge adds them to the owner's rows (integer adds: order-independent).
 *    flags (int32[1], caller-cleared): bit 0 a send segment overflowed cap_pair, bit 1 the local arrays did.
 *    counts: (world, 8) int32 rows per view of every rank (all-gathered view totals of iso_splat_front).
 *    Limits: world <= 64, 1..8 views.  iso_splat_band_export expects num_points[v] <= max_rows_per_view; rows of a view
 *    beyond (ceil(max_rows_per_view / 512) + 1) * 512 are not looked at (not sent, NOT flagged).  After a clip the
 *    delivered records are a prefix: a segment keeps its first cap_pair records (the header counts of the views past the
 *    cut are 0), the local arrays their first cap_local rows.  iso_splat_band_return writes the slots of the local rows
 *    only: the slot of a record that was dropped at cap_local keeps the caller's value, which iso_splat_band_merge then
 *    adds -- keep `ret` zero there if such a record is to contribute nothing (a record dropped at cap_pair has no slot).
 *    Outputs need no initial value; nothing outside the extents above is written (tests/test_exchange_gpu.py).    */
int64_t iso_splat_band_segment_floats(int64_t cap_pair);
int64_t iso_splat_band_export_workspace_bytes(int64_t max_rows_per_view, int n_views, int world);
int iso_splat_band_export(const float* ndc, const float* ellipse, const float* radii, const float* scaler,
                          const float* features, const int64_t* first_idx, const int64_t* num_points,
                          int n_views, int64_t max_rows_per_view, const int32_t* counts, int world, int rank,
                          int image_size, int image_width, int64_t cap_pair, float* send, int32_t* sent_row,
                          int64_t* acc_own, uint8_t* vis_own, int64_t* gid_first, int64_t* first_global,
                          int64_t* num_global, int32_t* flags, void* workspace, int64_t workspace_bytes,
                          void* stream);
int iso_splat_band_import(const float* recv, int world, int n_views, int64_t cap_pair, int64_t cap_local,
                          float cutoff, float* ndc, float* ellipse, float* cutoff_out, float* radii,
                          float* scaler, float* features, int32_t* gid, int32_t* origin, int64_t* acc_local,
                          uint8_t* vis_local, int64_t* first_local, int64_t* num_local, int32_t* place,
                          int32_t* flags, void* stream);
int iso_splat_band_remap(const int32_t* idx_local, const int32_t* gid, int n_views, int64_t view_pixels,
                         int64_t band_pixel0, int64_t band_pixels, int points_per_pixel, int32_t* idx_global,
                         void* stream);
int iso_splat_band_return(const int64_t* acc_local, const uint8_t* vis_local, const int32_t* origin,
                          const int64_t* first_local, const int64_t* num_local, int n_views, int64_t cap_local,
                          int64_t* ret, void* stream);
int iso_splat_band_merge(const int64_t* back, const int32_t* sent_row, int world, int n_views,
                         int64_t max_rows_per_view, int64_t cap_pair, int64_t* acc_own, uint8_t* vis_own,
                         const void* workspace, void* stream);
/* iso_splat_median_radius in pieces: pass 0, 1, 2 count the caller's rows into the pass's histograms (the slice
 * workspace + pass * iso_splat_median_pass_words(n_clouds) words of that many words), N ranks sum that slice over
 * the ranks before the next piece; iso_splat_median_final resolves and leaves the workspace zeroed.            */
int64_t iso_splat_median_pass_words(int n_clouds);
int iso_splat_median_pass(int pass, const float* radii, const uint8_t* visible, const int64_t* first_idx,
                          const int64_t* num_pts, int n_clouds, int64_t max_pts, void* workspace,
                          int64_t workspace_bytes, void* stream);
int iso_splat_median_final(void* workspace, int n_clouds, float radii_s, float* search_radius_out, void* stream);

/* ----------------------------------------------------------------------
 * G. Chamfer distance between point clouds (csrc/chamfer.hip)
 *    replaces pytorch3d.loss.chamfer_distance (CUDA-only, not vendored) where the reference calls it:
 *      evaluation.py:119-122, :169-172     chamfer_p / chamfer_n of the extracted iso-points
 *      DSS/training/trainer.py:256         the validation metric train_mvr.py:196 selects checkpoints by
 *    Both entries enqueue on `stream` and do not synchronise; no float atomics: two runs give the same bits.
 *
 * iso_chamfer_nearest: for every valid row i of x (N,P1,3) the exact nearest point of cloud y (N,P2,3), whose grid
 * (sorted_y, sorted_idx_y, off, grid_params) comes from the build calls of section B at an infinite radius:
 *   d2_out (N,P1) f32 = (dx*dx + dy*dy) + dz*dz (f32, no FMA contraction), ties -> the lower index of y;
 *   d2_out and nterm_out may be NULL (the loss needs the indices and the sums only);
 *   idx_out (N,P1) i32; with normals (both or neither; (N,P,3), any length) nterm_out (N,P1) =
 *   1 - |cos(x_normals[i], y_normals[idx[i]])|, cos = dot / (max(|a|, 1e-6) max(|b|, 1e-6)).
 * Rows i >= x_lengths[n], rows with a NaN coordinate and every row of a cloud whose y is empty get d2 = 0, idx = -1,
 * nterm = 0.  sums_out (N,2) = {sum d2, sum nterm} per cloud: per-workgroup partial sums, added in a fixed order
 * (64 contiguous chunks, each in index order, then the chunks in order).
 * workspace: iso_chamfer_nearest_workspace_bytes(N, P1, P2), 16-B aligned.                                          */
int64_t iso_chamfer_nearest_workspace_bytes(int n_clouds, int64_t p1, int64_t p2);
int iso_chamfer_nearest(const float* x, const int64_t* x_lengths, const float* sorted_y,
                        const int32_t* sorted_idx_y, const int64_t* y_lengths, const int32_t* off,
                        const float* grid_params, const float* x_normals, const float* y_normals,
                        float* d2_out, int32_t* idx_out, float* nterm_out, float* sums_out, int n_clouds,
                        int64_t p1, int64_t p2, int64_t g_stride, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* iso_chamfer_backward: gradient of
 *   sum_n g_dx[n] sum_i d2(x_i, y[idx_x[i]]) + g_dy[n] sum_j d2(y_j, x[idx_y[j]])
 * (and of the same two sums of the normal terms, scaled by g_nx / g_ny) w.r.t. both clouds and both normal tensors, in
 * one call: both sides share every launch (zero, count, three scan phases, fill, two gradient kernels).  Indices are
 * constants, so the normal terms have no gradient w.r.t. positions.  idx_x (N,P1), idx_y (N,P2): the i32 results of
 * iso_chamfer_nearest in the two directions (-1 = no term); g_* (N) f32 carry weights, the length and batch
 * normalisation and the upstream gradient.
 *   grad_x[i] = 2 g_dx (x_i - y[idx_x[i]]) + 2 g_dy sum_{j: idx_y[j] = i} (x_i - y_j)        (grad_y likewise)
 * The second part is a gather: the other cloud's indices are counting-sorted by target (integer atomics,
 * iso_prefix_sum) and each target's list is summed in ascending j by its own lane (up to 8 entries) or by one wave
 * (sorted up to 1024 entries, beyond that a strided scan of the index row): a fixed order.  Rows beyond a cloud's length
 * get 0.  grad_x or grad_y may be NULL: that side is skipped; grad_*_normals may be NULL (a normal gradient needs its
 * cloud's position gradient buffer).  workspace: iso_chamfer_backward_workspace_bytes(N, P1, P2), 16-B aligned.        */
int64_t iso_chamfer_backward_workspace_bytes(int n_clouds, int64_t p1, int64_t p2);
int iso_chamfer_backward(const float* x, const float* y, const int64_t* x_lengths, const int64_t* y_lengths,
                         const int32_t* idx_x, const int32_t* idx_y, const float* g_dx, const float* g_dy,
                         const float* x_normals, const float* y_normals, const float* g_nx, const float* g_ny,
                         float* grad_x, float* grad_y, float* grad_x_normals, float* grad_y_normals,
                         int n_clouds, int64_t p1, int64_t p2, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ----------------------------------------------------------------------
 * H. Point-to-mesh face distances (csrc/pfdist.hip)
 *    replaces pytorch3d.loss.point_mesh_face_distance and pytorch3d.loss.point_mesh_distance.point_face_distance
 *    (CUDA-only, not vendored) where the reference calls them:
 *      evaluation.py:78, :123-126, :146, :173-176   pf_dist of the checkpoints' and the final mesh
 *      DSS/training/losses.py:536-598                SignedDistanceLoss: the distance it signs
 *    Clouds and meshes are PACKED: points (P,3), tris (T,3,3) f32, with first (N) and len (N) i64 per cloud / mesh; point
 *    and face indices are packed indices.  All entries enqueue on `stream` and do not synchronise; no float atomics: two
 *    runs give the same bits.
 *
 * d2(p, t): the squared distance from p to the closed triangle t, evaluated as |p - (b0 v0 + b1 v1 + b2 v2)|^2 in f32
 * without FMA contraction: a pure function of the pair.  A triangle of area > min_triangle_area whose plane projection
 * of p has no negative weight is measured there, every other pair by the triangle's three edges; a triangle without
 * area gives no NaN.
 *
 * iso_pfdist_prepare: what the searches need of their inputs, either half optional (NULL output):
 *   points_padded_out (N,p_stride,3): the clouds, one row each (the input of the point grid);
 *   centroids_out (N,t_stride,3): the faces' centroids, one row per mesh (the input of the face grid); radius_out (T):
 *   R_t = the largest centroid-to-vertex distance, rounded up; rmax_out (N): the largest R_t of each mesh.
 *
 * iso_pfdist_forward, direction 0 (point -> face): for every point the nearest face of its own mesh, ties -> the lower
 * face index.  The grid (sorted_targets, sorted_idx, off, grid_params; section B at an infinite radius) is built on the
 * CENTROIDS; after shell rho of the walk every unseen face is at least ring_reach(rho) - R_max away, which is the stop
 * rule.  One face far larger than a cell drives every walk of its mesh toward brute force; the result stays exact.
 * direction 1 (face -> point): for every face the nearest point of its own cloud, ties -> the lower point index; the
 * grid is built on the padded POINTS, the walk starts at the face's centroid and stops once
 * sqrt(best) + R_t <= ring_reach(rho).  d2_out (Q) f32, idx_out (Q) i32 (packed index; a query without targets: d2 = 0,
 * idx = -1), sums_out (N) = the sum of d2 over the cloud's points / the mesh's faces: per-workgroup partial sums added in
 * a fixed order.  p_stride / t_stride >= every len.  workspace: iso_pfdist_forward_workspace_bytes(direction, N,
 * the queries' stride, the targets' stride), 16-B aligned.
 *
 * iso_pfdist_backward: gradient of sum_q weights[q] d2(q, idx[q]) of one direction w.r.t. the points and the
 * triangles, indices constant: with r = p - c, d d2 / d p = 2 r and d d2 / d v_k = -2 b_k r.  The queries' side is
 * written directly; the targets' side is a gather over lists counting-sorted by target (integer atomics,
 * iso_prefix_sum), each list summed in ascending query order by its own lane (up to 8 entries) or by one wave (sorted up
 * to 1024 entries, beyond that a strided scan of idx).  grad_points (P,3) or grad_tris (T,9) may be NULL: that side is
 * skipped.  workspace: iso_pfdist_backward_workspace_bytes(direction, P, T), 16-B aligned.                          */
int iso_pfdist_prepare(const float* points, const int64_t* pts_first, const int64_t* pts_len, const float* tris,
                       const int64_t* tris_first, const int64_t* tris_len, int n_clouds, int64_t n_points,
                       int64_t n_tris, int64_t p_stride, int64_t t_stride, float* points_padded_out,
                       float* centroids_out, float* radius_out, float* rmax_out, void* stream);
int64_t iso_pfdist_forward_workspace_bytes(int direction, int n_clouds, int64_t q_stride, int64_t target_stride);
int iso_pfdist_forward(int direction, const float* points, const int64_t* pts_first, const int64_t* pts_len,
                       const float* tris, const int64_t* tris_first, const int64_t* tris_len,
                       const float* sorted_targets, const int32_t* sorted_idx, const int32_t* off,
                       const float* grid_params, const float* centroids, const float* radius, const float* rmax,
                       float min_triangle_area, float* d2_out, int32_t* idx_out, float* sums_out, int n_clouds,
                       int64_t n_points, int64_t n_tris, int64_t p_stride, int64_t t_stride, int64_t g_stride,
                       void* workspace, int64_t workspace_bytes, void* stream);
int64_t iso_pfdist_backward_workspace_bytes(int direction, int64_t n_points, int64_t n_tris);
int iso_pfdist_backward(int direction, const float* points, const float* tris, const int32_t* idx,
                        const float* weights, float min_triangle_area, float* grad_points, float* grad_tris,
                        int64_t n_points, int64_t n_tris, void* workspace, int64_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------
 * I. Sampling points on meshes (csrc/mesh_sample.hip)
 *    replaces pytorch3d.ops.sample_points_from_meshes (CUDA-only, not vendored) where the reference calls it:
 *      evaluation.py:113, :164                    the points and normals that chamfer_p / chamfer_n / pf_dist grade
 *      scripts/create_mvr_data_from_mesh.py:171   the ground-truth cloud of a scene
 *      tests/test_projection.py:347               the reference's own projection test
 *    Meshes are PACKED as in section H: tris (T,3,3) f32 with first (N) and len (N) i64 per mesh (rows outside the packed
 *    array are ignored); face indices are packed indices.  Limits: T < 2^31 and N * S < 2^31, refused beyond.  The device
 *    entries enqueue on `stream` and do not synchronise; no float atomics: two runs give the same bits.
 *
 * Per face, in f32 without FMA contraction: m = (v1 - v0) x (v2 - v0), area = 0.5f * sqrtf((m.x*m.x + m.y*m.y) + m.z*m.z),
 * unit normal = m / max(|m|, 2.220446e-16f).  iso_mesh_face_areas writes areas_out (T) and normals_out (T,3); either may
 * be NULL.
 *
 * iso_mesh_sample: S samples on each of N meshes.  Sample s of mesh n takes the four words r0..r3 of Philox4x32-10 with
 * key = (seed & 0xffffffff, seed >> 32) and counter = (s & 0xffffffff, s >> 32, n, 0):
 *   uf = ((uint64(r0) << 21) | (r1 >> 11)) * 2^-53 (f64), u = (r2 >> 8) * 2^-24, v = (r3 >> 8) * 2^-24 (f32), all exact.
 * C is the inclusive running sum of the mesh's f32 areas accumulated in f64 (a thread adds 8 faces in order, the 256
 * threads of a tile of 2048 faces and then the tiles are added in order: a fixed shape, C never descends and a face
 * without area has the C of its predecessor), A its last entry.  The face is the first f of the mesh with C[f] > uf * A
 * (a face without area is never chosen); the point is (w0 v0 + w1 v1) + w2 v2 per component with sq = sqrtf(u),
 * w0 = 1 - sq, w1 = sq * (1 - v), w2 = sq * v.  So a sample depends on (seed, n, s) and its mesh only: not on S, not on
 * the other meshes, not on a launch shape.
 *   points_out (N,S,3); normals_out (N,S,3) = the face's unit normal, face_idx_out (N,S) i32 = the packed face row,
 *   bary_out (N,S,3) = (w0, w1, w2): each of the three may be NULL.
 * A mesh without faces or whose A is not a positive finite number gets points = normals = bary = 0 and face_idx = -1.
 * Launches: areas, the scan (three), the draw.  workspace: iso_mesh_sample_workspace_bytes(N, T), 16-B aligned.
 *
 * iso_mesh_sample_backward: gradient w.r.t. the triangles of sum_q g_points[q] . point_q + g_normals[q] . normal_q over
 * the n_rows = N * S samples, faces and weights constant (face_idx < 0: no term):
 *   grad_tris[f,k,:] = sum_{q: face_idx[q] = f} bary[q,k] g_points[q]   and, with G = sum_{q: face_idx[q] = f} g_normals[q],
 *   dm = (G - n (n.G)) / |m| (G / 2.220446e-16f where |m| is below that), de1 = e2 x dm, de2 = dm x e1:
 *   v1 += de1, v2 += de2, v0 -= de1 + de2.
 * The sums are the gather of sections G and H: lists counting-sorted by face (integer atomics, iso_prefix_sum), each
 * summed in ascending sample order by its own lane (up to 8 entries) or by one wave (sorted up to 1024 entries, beyond
 * that a strided scan of face_idx).  g_normals may be NULL; faces nobody chose get 0.
 * workspace: iso_mesh_sample_backward_workspace_bytes(T, N * S), 16-B aligned.
 *
 * iso_mesh_sample_draw: a HOST function (no device, no stream): out_words[4] = r0..r3 of sample `sample` of mesh `mesh`
 * by the very routine the kernel runs, for tests that pin the generator.                                              */
int iso_mesh_face_areas(const float* tris, int64_t n_tris, float* areas_out, float* normals_out, void* stream);
int64_t iso_mesh_sample_workspace_bytes(int n_meshes, int64_t n_tris);
int iso_mesh_sample(const float* tris, const int64_t* tris_first, const int64_t* tris_len, int n_meshes,
                    int64_t n_tris, int64_t n_samples, int64_t seed, float* points_out, float* normals_out,
                    int32_t* face_idx_out, float* bary_out, void* workspace, int64_t workspace_bytes, void* stream);
int64_t iso_mesh_sample_backward_workspace_bytes(int64_t n_tris, int64_t n_rows);
int iso_mesh_sample_backward(const float* tris, const int32_t* face_idx, const float* bary, const float* g_points,
                             const float* g_normals, float* grad_tris, int64_t n_tris, int64_t n_rows,
                             void* workspace, int64_t workspace_bytes, void* stream);
int iso_mesh_sample_draw(int64_t seed, int mesh, int64_t sample, uint32_t* out_words);

/* ----------------------------------------------------------------------
 * J. Sign of the point-to-mesh distance (csrc/pfsign.hip)
 *    replaces the inside test of the reference's SignedDistanceLoss (DSS/training/losses.py:536-598), which takes the
 *    parity of four rasterised depth layers of pytorch3d's CUDA-only MeshRasterizer under each point.  Here the sign is
 *    exact by orientation: the angle-weighted pseudonormal test of Baerentzen & Aanaes.  With c the closest point of the
 *    mesh to p and N the pseudonormal of the feature c lies on, the sign is that of (p - c) . N:
 *      face interior   the face's unit normal (v1 - v0) x (v2 - v0) / |.|
 *      edge            the sum of the unit normals of all faces that hold both end vertices
 *      vertex          the sum over the incident corners of corner angle * the corner's face normal
 *    Outward-wound faces give -1 inside and +1 outside; reversing the winding reverses the sign.  Meshes are PACKED:
 *    verts (V,3) f32, faces (F,3) i64 rows of verts (a face with a row outside [0, V) counts as a face without area),
 *    tris (F,3,3) f32 = verts[faces] as section H takes them.  Limits: V < 2^31 - 1, F < (2^31 - 1) / 3, P < 2^31 - 1, refused beyond.
 *    The device entries enqueue on `stream` and do not synchronise; no float atomics: two runs give the same bits.
 *
 * iso_pfsign_normals: in f32 without FMA contraction, per face m = (v1 - v0) x (v2 - v0), n = m / |m|; a face whose |m| is
 * not a positive finite number gets n = 0 and angles 0, so it contributes nothing anywhere and gives no NaN.  The angle of
 * corner k is atan2f(|a x b|, a . b) with a = v[k+1] - v[k], b = v[k+2] - v[k] (indices mod 3).
 *   face_normals_out (F,3) = n;
 *   vert_normals_out (V,3) = sum of angle * n over the corners at the vertex, in ascending corner order (corner = 3 f + k):
 *   the corner lists are the gather of sections G to I (counting sort on integer atomics, iso_prefix_sum), a list summed by
 *   its own lane (up to 8 corners) or by one wave (sorted up to 1024, beyond that a strided scan of the corners);
 *   edge_normals_out (F,3,3): slot k of face f is the edge from its vertex k to its vertex k + 1 mod 3 and holds the sum of
 *   n_g over all faces g that hold both end vertices, in ascending g: a boundary edge gets its one face, a non-manifold
 *   edge all of its faces; a slot whose two ends are the same vertex gets 0.
 * The vectors are not normalised: only their direction is used.  A mesh without faces gets zero vectors.
 * workspace: iso_pfsign_normals_workspace_bytes(V, F), 16-B aligned.
 *
 * iso_pfsign_sign: one lane per point.  idx (P) i32 is the packed nearest face as iso_pfdist_forward (direction 0) wrote
 * it, -1 = none; min_triangle_area the value that search ran with.  The lane evaluates section H's d2(p, t) again for the
 * closest point's weights (b0, b1, b2) and reads the feature off the weights that are exactly zero (the edge branch of
 * d2 produces exact zeros and ones): none -> the face; one -> the edge opposite that vertex; two -> the vertex that is
 * left.  c = (b0 v0 + b1 v1) + b2 v2, sign = ((p - c) . N < 0) ? -1 : +1: a zero product, a zero N and a point without a
 * face give +1.
 *   sign_out (P) f32; feature_out (P) i32: 0 = face, 1..3 = edge slot + 1, 4..6 = corner + 4, -1 = no face.
 *
 * iso_pfsign_pair: a HOST function (no device, no stream): one point (3) against one triangle (9) by the very routines
 * the kernels run: d2_out[1], weights_out[3], feature_out[1], for tests that pin the arithmetic.                      */
int64_t iso_pfsign_normals_workspace_bytes(int64_t n_verts, int64_t n_faces);
int iso_pfsign_normals(const float* verts, const int64_t* faces, int64_t n_verts, int64_t n_faces,
                       float* face_normals_out, float* edge_normals_out, float* vert_normals_out, void* workspace,
                       int64_t workspace_bytes, void* stream);
int iso_pfsign_sign(const float* points, const int32_t* idx, const float* tris, const int64_t* faces,
                    const float* face_normals, const float* edge_normals, const float* vert_normals,
                    float min_triangle_area, float* sign_out, int32_t* feature_out, int64_t n_points, int64_t n_faces,
                    int64_t n_verts, void* stream);
int iso_pfsign_pair(const float* point, const float* tri, float min_triangle_area, float* d2_out, float* weights_out,
                    int32_t* feature_out);

/* ----------------------------------------------------------------------
 * K. The point-cloud regularisers of the splatting renderer (csrc/surface_loss.hip)
 *    replaces the bodies of SurfaceLoss / ProjectionLoss / RepulsionLoss (DSS/training/losses.py:149-515; Eq. 10-15 of the
 *    DSS paper): two normal mollifications and the two losses over the K nearest OTHER points of every point, which the
 *    reference composes from about twenty torch ops on (N,P,K) and (N,P,K,3) temporaries.
 *
 *    Notation.  Cloud b has L_b valid points; p_i is row i; j = idx[i,k] and d_k = dists[i,k] (squared, ascending,
 *    k = 0..K-1; section B's iso_frnn_query_others), d_0 the nearest other point; fs = filter_scale; inv_sigma2 =
 *    1 / sharpness_sigma^2 (the caller's division); sd(x) = sign(x) max(|x|, 1e-17) with sd(0) = 1e-17
 *    (DSS/utils/mathHelper.py:14-18); u(v) = v / max(|v|, 1e-12).  All f32 without FMA contraction, expf the accurate one.
 *      phi_ik = max(0, 1 - d_k / (((2 d_0) fs) fs))^4                         (:262-276)
 *      nu_ik  = exp(-|u(m_j) - u(m_i)|^2 inv_sigma2)  for a normal field m     (:225-248)
 *    Lanes.  One lane per neighbour slot, 32 lanes per row, two rows per wave: a row's indices are one 256-B read, its
 *    distances one 128-B read, the neighbours' vectors 12-B gathers.  Every sum over k is the same xor butterfly over the
 *    32 lanes (slots >= K, and slots whose index is outside [0), add zeros): a fixed order, no atomics, two
 *    runs give the same bits.  idx / dists rows start at idx + row * idx_row_stride and dists + row * dists_row_stride
 *    (row = n * p_stride + i), so columns 1.. of a wider query result need no copy.
 *    K outside [1,32] -> ISO_ERR_UNSUPPORTED; null pointers, negative sizes, row strides < K -> ISO_ERR_INVALID.
 *    Every cloud needs L_b >= K + 1 (every slot filled); the callers check that on the host.  Clouds with duplicate
 *    points are undefined: d_0 = 0 makes phi 0/0, as in the reference.
 *
 * iso_surfloss_mollify: out_i = sum_k phi_ik [nu_ik] in_j / sd(sum_k phi_ik [nu_ik]); nu (from the field `in` itself) is
 *   included when use_normal_w != 0.  The reference's two calls: n0 -> n1 without nu (:332), n1 -> n2 with nu (:337-342).
 *   Neither sum is masked by the ball test, as in the reference.  Rows i >= L_b are written as zeros.  in != out.
 *
 * iso_surfloss_forward: x_j = nbr_points[n, j] ((N, 3): the points the neighbour lists were built on), or
 *   knn[n, i, k] when knn != NULL ((N, p_stride, K, 3) contiguous).  With nu from n1:
 *      ball_ik = d_k > (fs d_0) 2                                             (:349-351)
 *      w_ik    = phi_ik nu_ik where not ball_ik, else 0
 *      s_ik    = <x_j - p_i, n2_j>
 *   projection (:367-403):  D_i = sum w s / sd(sum w);  proj_i = D_i^2;  dproj_i/dp_i = 2 D_i (-sum_k w_ik n2_j / sd(sum w))
 *   repulsion (:462-515):   q_i = p_i + sum_k (s_ik w_ik) n2_j / sd(sum w)
 *                           sig_ik = exp(-|x_j - q_i|^2 L_b / 2);  dens_i = 1 + sum_k sig_ik     (all K slots, unmasked)
 *                           W_ik = nu_ik sig_ik dens_i where not ball_ik, else 0
 *                           rep_i = -sum_k |q_i - x_j|^2 W_ik / sd(sum W)
 *                           g_i = -sum_k 2 (q_i - x_j) W_ik / sd(sum W);  drep_i/dp_i = g_i - sum_k w_ik n2_j <n2_j, g_i> / sd(sum w)
 *   The bandwidth L_b / 2 is PER CLOUD: the reference's expression broadcasts an (N,) tensor against (N,P,K) and so only runs
 *   for one cloud; per cloud is what it means.  Weights, normals and neighbour positions carry no gradient in the reference
 *   (no_grad / detach), so a row's gradient touches its own point only: the two (N,P,3) gradient arrays ARE the backward
 *   pass, up to a row-wise scale.  outputs: bit 0 (ISO_SURFLOSS_PROJECTION) proj_out (N,P) and, with bit 2, grad_proj_out
 *   (N,P,3); bit 1 (ISO_SURFLOSS_REPULSION) rep_out and grad_rep_out likewise; bit 2 (ISO_SURFLOSS_GRADIENTS).  A value
 *   is the same bits whichever other outputs are asked for.  Rows i >= L_b are written as zeros.                        */
#define ISO_SURFLOSS_PROJECTION 1
#define ISO_SURFLOSS_REPULSION 2
#define ISO_SURFLOSS_GRADIENTS 4
int iso_surfloss_mollify(const float* normals_in, const int64_t* idx, int64_t idx_row_stride, const float* dists,
                         int64_t dists_row_stride, const int64_t* lengths, int n_clouds, int64_t p_stride, int K, float filter_scale, float inv_sigma2, int use_normal_w,
                         float* normals_out, void* stream);
int iso_surfloss_forward(const float* points, const float* nbr_points, const float* knn, const float* n1, const float* n2,
                         const int64_t* idx, int64_t idx_row_stride, const float* dists, int64_t dists_row_stride,
                         const int64_t* lengths, int n_clouds, int64_t p_stride, int K,
                         float filter_scale, float inv_sigma2, int outputs, float* proj_out, float* rep_out,
                         float* grad_proj_out, float* grad_rep_out, void* stream);

/* ----------------------------------------------------------------------
 * L. Even sampling: Poisson-disk elimination (csrc/disk.hip)
 *    serves the places where the reference turns a mesh into the cloud it uses and asks for an EVEN sampling:
 *      config.py:227                    trimesh.sample.sample_surface_even: the initial iso-points of the combined model
 *      DSS/training/trainer.py:255      sample_surface_even of the generated mesh, graded by chamfer_distance (validation)
 *      DSS/utils/dataset.py:123         pcu.sample_mesh_poisson_disk: the ground-truth cloud
 *    trimesh and point_cloud_utils are third-party and not part of the reference tree; bit parity with either is not
 *    claimed.  The definition here is exact, maximal and stable under a longer draw (trimesh's one-shot degree rule is
 *    neither maximal nor prefix-stable; pcu measures along the surface).
 *
 *    Definition.  Cloud n has L_n samples p_0 .. p_{L_n - 1} and a radius r_n.  Two samples CONFLICT iff d2(i, j) <= r2 with
 *    d2 = (dx*dx + dy*dy) + dz*dz in f32 without FMA contraction (section B's expression) and r2 = r_n * r_n in f32.  Sample s
 *    is KEPT iff no kept sample j < s conflicts with it; a sample marked invalid on entry is removed and blocks nobody:
 *    serial dart throwing in index order.  So the kept set is an exact integer result; no two kept samples conflict; every
 *    removed valid sample has a kept conflicting sample of lower index; and the kept set of the first k samples is the same
 *    whether or not more samples follow.  Coordinates must be finite.
 *
 *    Parallel form.  One state byte per sample (UNDECIDED, KEEP, REMOVED).  A round visits every UNDECIDED s and reads the
 *    state of every conflicting j < s: any KEEP -> REMOVED; else any UNDECIDED -> unchanged; else KEEP.  States move only
 *    from UNDECIDED to a final value and are finalised only from final states below them, so rounds update in place, a
 *    stale read only delays a decision, and the fixed point is the serial result whatever the launch shape or the timing
 *    (csrc/disk.hip's header has the argument).  Every round finalises at least the lowest UNDECIDED sample of each cloud.
 *
 *    The grid is section B's, built on the cloud itself at this radius (make_grid_density, insert_points, scan_cells,
 *    counting_sort): sorted_points (N,P,3), sorted_idx (N,P), off (N,g_stride), grid_params (N,8).  The device entries
 *    enqueue on `stream` and do not synchronise.  Limit: N * P < 2^31 - 1, refused beyond.  All three calls of one
 *    elimination share one workspace of iso_disk_workspace_bytes(N, P) bytes, 16-B aligned, untouched in between.
 *
 * iso_disk_begin: packs the grid's records and sets the state bytes: row i of cloud n is UNDECIDED if i < lengths[n]
 *   (lengths NULL: P) and valid[n,i] != 0 (valid (N,P) u8, NULL: all valid), else REMOVED; zeroes the round counters.
 * iso_disk_rounds: enqueues rounds first_round .. first_round + n_rounds - 1 (the caller counts the rounds of one
 *   elimination from 0 over its calls; n_rounds >= 1) and then writes *left (one i32 on the device) = the number of samples
 *   still UNDECIDED after the last of them.  A round whose predecessor left none returns at once.  radius (N) f32.
 * iso_disk_select: the stable compaction.  sel_out (N,s_out) i32 = the indices of the first s_out kept samples of each
 *   cloud in ascending order, -1 beyond; kept_out (N) i64 = min(number kept, s_out); mask_out (N,P) u8 = 1 where kept
 *   (may be NULL).  A scan: integer work only, nothing order-dependent.  Valid once *left is 0.
 * iso_disk_area_radius: radius_out[n] = (float) sqrt(A_n / (3 n_samples)), A_n the sum in f64 (fixed order) of the f32
 *   areas (section I) of mesh n's packed faces; 0 for a mesh whose A_n is not a positive finite number.                */
int64_t iso_disk_workspace_bytes(int n_clouds, int64_t p_stride);
int iso_disk_begin(const float* sorted_points, const int32_t* sorted_idx, const int64_t* lengths, const uint8_t* valid,
                   int n_clouds, int64_t p_stride, void* workspace, int64_t workspace_bytes, void* stream);
int iso_disk_rounds(const int64_t* lengths, const int32_t* off, const float* grid_params, const float* radius,
                    int n_clouds, int64_t p_stride, int64_t g_stride, int first_round, int n_rounds, int32_t* left,
                    void* workspace, int64_t workspace_bytes, void* stream);
int iso_disk_select(int n_clouds, int64_t p_stride, int64_t s_out, uint8_t* mask_out, int32_t* sel_out, int64_t* kept_out,
                    void* workspace, int64_t workspace_bytes, void* stream);
int iso_disk_area_radius(const float* areas, const int64_t* tris_first, const int64_t* tris_len, int n_meshes,
                         int64_t n_tris, int64_t n_samples, float* radius_out, void* stream);

/* ----------------------------------------------------------------------
 * M. Mesh rasterisation: faces, depth and barycentrics per pixel (csrc/mesh_raster.hip)
 *    serves the places where the reference renders a ground-truth mesh through pytorch3d's MeshRasterizer:
 *      scripts/create_mvr_data_from_mesh.py:143-216   every synthetic training set: MeshRasterizer(faces_per_pixel=5,
 *                                                     blur_radius=0) -> HardFlatShader -> RGBA, mask, dense depth
 *      DSS/training/losses.py:550-578                 SignedDistanceLoss: four depth layers at 256 x 256
 *      tests/test_data.py, tests/test_dvr_camera.py   the reference's own tests
 *    = pytorch3d.renderer.mesh.rasterize_meshes at blur_radius = 0 (nothing else is ever passed), no backward pass.
 *
 *    Inputs, as rasterize_meshes has them after its transform: face_verts (F,3,3) f32 packed over N meshes, x and y in NDC
 *    (+X left, +Y up), z the view-space depth; first_idx (N) / num_faces (N) i64, first_idx non-decreasing (packed order);
 *    a square image of side S; K = faces_per_pixel in 1..8.
 *
 *    The rule (float32, no FMA contraction, IEEE division; tests/mesh_raster_oracle.py states it in float64 and float32).
 *    Centre of output row r, column c: X = 1 - (2c+1)/S, Y = 1 - (2r+1)/S (pytorch3d's PixToNdc with its x/y flip).
 *    edge(a, b; q) = (qx - ax)(by - ay) - (qy - ay)(bx - ax), in this difference form.  area = edge(v0, v1; v2).
 *    A face is skipped if |area| <= 1e-8, if its largest z is < 0, if any of its nine numbers is not finite, or if
 *    cull_backfaces is set and area < 0 (area > 0 is counter-clockwise in the displayed image).
 *    w0 = edge(v1, v2; p) / area, w1 = edge(v2, v0; p) / area, w2 = edge(v0, v1; p) / area; the pixel is inside iff all
 *    three are > 0 (strict: a centre exactly on a shared edge belongs to neither face, as in pytorch3d).
 *    b = w; with perspective_correct t = (w0 z1 z2, w1 z0 z2, w2 z0 z1), b = t / ((t0 + t1) + t2).
 *    pz = (b0 z0 + b1 z1) + b2 z2; the pair is skipped if pz < 0 or pz is not finite.
 *    dist = -(smallest squared distance in NDC xy from p to the segments v0v1, v0v2, v1v2; a segment shorter than
 *    1e-4 (l2 <= 1e-8) counts as its second end point).
 *    Per pixel the K smallest pairs by the total order (pz, packed face index) ascending: equal depth goes to the lower
 *    index.  pix_to_face (N,S,S,K) i64, zbuf (N,S,S,K), bary (N,S,S,K,3), dists (N,S,S,K) f32; an empty slot holds -1 in
 *    all four.  Every pixel of every mesh is written.
 *    Deviations from pytorch3d: no 1e-8 added to the denominators (area, t0 + t1 + t2) -- those faces and pairs are skipped
 *    instead; NaN / inf faces are skipped; no max_faces_per_bin -- a tile's face list has no capacity and cannot overflow.
 *
 *    Three passes around one caller-side read of the pair total, the shape of the splat forward (section D):
 *      iso_meshraster_count  : tile_cnt (N*T*T i32, zero on entry, T = iso_splat_tiles_per_side(S)) += faces whose clamped
 *                               bounding box touches the 16x16 tile; integer atomics only;
 *      caller                 : iso_splat_tile_offsets(tile_cnt, tile_off, tile_cursor, N*T*T + 1), total = tile_off[N*T*T],
 *                               allocate pairs (i32, >= total);
 *      iso_meshraster_fill   : the same walk, face indices into pairs; the order inside a tile's list is arbitrary and the
 *                               result does not depend on it;
 *      iso_meshraster_pixels : one 256-lane workgroup per tile, one pixel per lane, the tile's faces staged through LDS
 *                               256 at a time, the K nearest (pz, id) of the pixel in registers.  Compiled for K = 1, 4
 *                               and 8 (iso_meshraster_form); another K runs on the next form up and writes its first K.
 *    Refused with an error code, nothing launched: K outside 1..8, S < 1, N * S * S * K >= 2^31, F >= 2^31, negative
 *    sizes, null pointers where work exists.  N = 0, F = 0 and meshes without faces are not errors (pixels hold -1).
 *    (The entries are iso_meshraster_*, in one word: the prefix iso_mesh_ is section I's, the mesh sampler's.)        */
int iso_meshraster_form(int faces_per_pixel);
int iso_meshraster_count(const float* face_verts, const int64_t* first_idx, const int64_t* num_faces, int n_meshes,
                          int64_t n_faces, int image_size, int cull_backfaces, int32_t* tile_cnt, void* stream);
int iso_meshraster_fill(const float* face_verts, const int64_t* first_idx, const int64_t* num_faces, int n_meshes,
                         int64_t n_faces, int image_size, int cull_backfaces, int32_t* tile_cursor, const int32_t* tile_off,
                         int32_t* pairs, int64_t pair_capacity, void* stream);
int iso_meshraster_pixels(const float* face_verts, int n_meshes, int64_t n_faces, int image_size, int faces_per_pixel,
                           int perspective_correct, const int32_t* tile_off, const int32_t* pairs, int64_t pair_capacity,
                           int64_t* pix_to_face, float* zbuf, float* bary, float* dists, void* stream);

/* ----------------------------------------------------------------------
 * N. Mesh extraction: the level set of a sampled SDF as an indexed triangle mesh (csrc/mesh_extract.hip)
 *    stands where the reference copies the volume to the host for skimage.measure.marching_cubes_lewiner:
 *      DSS/utils/__init__.py:569-655                  get_surface_high_res_mesh (both of its extractions, :582 and :635),
 *                                                     called by Generator.generate_mesh (DSS/models/implicit_modeling.py:
 *                                                     680-700), DSS/training/trainer.py:201, :254, :723, :887,
 *                                                     generate_mvr.py:75 and test_dtu_points.py:289, :322
 *    Not Lewiner's marching cubes and not bit for bit skimage's: marching tetrahedra on the Kuhn split, exact and
 *    deterministic by construction, about twice as many faces (tests/mesh_extract_oracle.py restates the
 *    rule in numpy, float32 and float64).
 *
 *    The rule.  values (nx,ny,nz) f32, C-contiguous; grid point (i,j,k) has linear index p = (i ny + j) nz + k and lies at
 *    origin + (i,j,k) * spacing, each coordinate one f32 multiplication and one addition.  A point is INSIDE iff its value is
 *    finite and < iso; a value equal to iso, NaN and +-inf are outside.
 *    Every point owns 7 slots, the mesh edges that START at it, in the order +x, +y, +z, +xy, +xz, +yz, +xyz.  A slot exists
 *    if its far end is in the grid and is ACTIVE if exactly one of its ends is inside.  An active slot carries one vertex,
 *    pa + t (pb - pa) per coordinate with t = (iso - va) / (vb - va), a the owning (lower) end: float32, IEEE division, no
 *    FMA contraction; t = 0.5 if va or vb is not finite (never interpolated).  Vertex index = the exclusive scan of the
 *    active flags in (p, slot) order.
 *    A cell is cut into six tetrahedra around its diagonal 000-111: 000 -> +e_a -> +e_a+e_b -> 111 for the permutations
 *    (a,b,c) of the axes in lexicographic order; neighbouring cells share every face diagonal, so there are no cracks.  A
 *    tetrahedron with corners P0..P3 and 1 or 3 of them inside gives the triangle (AB, AC, AD), A the lone corner, B < C < D
 *    the others, XY the vertex on edge XY; with A < B inside and C < D outside the triangles (AC, AD, BD), (AC, BD, BC).
 *    The last two corners are swapped where needed for the right-hand normal to point to the outside corners (towards
 *    larger values); csrc/mesh_extract.hip derives the 16 cases at compile time.  Faces are ordered by cell (linear index of
 *    its lowest point), tetrahedron, triangle; face index = the exclusive scan of the cells' counts.  Zero-area faces
 *    (t = 0: a value on the level) are kept.  No atomics: the same input gives the same bits on every run and stream.
 *
 * iso_meshextract_workspace_bytes: 17 bytes per grid point (the slots' mask, two counts, two offsets) plus the tiles'
 *   partial sums and iso_prefix_sum's workspace; 0 for sizes outside the limits.  16-byte aligned.
 * iso_meshextract_count: pass 1 (4 x 4 x 64 tiles with a one-point halo through LDS), the 64-bit totals and the scan
 *   (iso_prefix_sum over both count rows).  totals (device, 2 x i64) = the number of vertices and of faces.  Enqueues on
 *   `stream`, does not synchronise.
 * iso_meshextract_emit: pass 2 on the workspace iso_meshextract_count left, same values and iso: verts (V,3) f32, faces
 *   (F,3) i32.  Reads `totals` back (16 bytes, synchronises the stream) and refuses capacities below them with
 *   ISO_ERR_INVALID; verts / faces may be NULL where the total is 0.  spacing > 0.
 * Limits: 2 <= nx, ny, nz (ISO_ERR_INVALID below) <= 1024 (ISO_ERR_UNSUPPORTED above); fewer than 2^31 vertices and fewer
 *   than 2^31 faces (ISO_ERR_UNSUPPORTED from iso_meshextract_emit; the totals themselves are exact).
 *   (The entries are iso_meshextract_*, in one word, as section M's are: the prefix iso_mesh_ is section I's.)         */
int64_t iso_meshextract_workspace_bytes(int nx, int ny, int nz);
int iso_meshextract_count(const float* values, int nx, int ny, int nz, float iso, int64_t* totals, void* workspace,
                           int64_t workspace_bytes, void* stream);
int iso_meshextract_emit(const float* values, int nx, int ny, int nz, float ox, float oy, float oz, float sx, float sy,
                          float sz, float iso, const int64_t* totals, float* verts, int64_t vert_capacity, int32_t* faces,
                          int64_t face_capacity, const void* workspace, int64_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------
 * O. Block-sparse mesh extraction: section N's rule over a list of bricks of grid points (csrc/mesh_extract_sparse.hip)
 *    Work and memory follow the surface's area, not the box; sides go up to 4096 (DESIGN.md 3.4k;
 *    tests/mesh_sparse_oracle.py restates this section in numpy).
 *
 *    The grid.  (nx,ny,nz) points, each n in [2, 4096].  The inside test, the 7 slots of a point, the Kuhn split, the 16
 *    triangle cases, the vertex's arithmetic and the winding are section N's, from the same text (csrc/mesh_tables.h).
 *    Bricks.  Brick b = (bx,by,bz) holds the grid points with index 8 b_d .. 8 b_d + 7 per axis, clipped by the grid; there
 *    are ceil(n_d / 8) bricks per axis.  CELL-BLOCK b holds the cells whose base (lowest) point lies in brick b.  A sparse
 *    volume is
 *      coords (S,3) i32       the listed bricks, sorted by linear brick index (bx nby + by) nbz + bz and unique,
 *      values (S,8,8,8) f32   values[s][i][j][k] at grid point 8 coords[s] + (i,j,k); entries outside the grid are ignored,
 *      cell_active (S) u8     non-zero: the cells of cell-block coords[s] are marched.
 *    Every grid point is stored once: no halo, no duplicated sample.  The caller GUARANTEES that for a cell-active b every
 *    brick b + {0,1}^3 that exists in the grid is in the list (the sampled set); the library does not check it (a triangle
 *    corner whose owner is missing gets index -1; nothing is read or written out of bounds).
 *    Live slots.  Slot s of point p (offset code(s) in {1..7}, x = 1, y = 2, z = 4) is contained in the cells with base
 *    p - d for the offsets d in {0,1}^3 with d & code(s) == 0; they lie in cell-block b or a lower neighbour b - {0,1}^3.
 *    The slot is LIVE iff at least one of those cells exists and lies in a cell-active block; by the guarantee both its ends
 *    are then sampled.  A live slot whose ends differ in the inside test carries a vertex.  A cell is marched iff it
 *    exists and its block is cell-active.
 *    Order.  Vertices by brick in list order, then local point index (i 8 + j) 8 + k, then slot; faces by cell-block in list
 *    order, then local cell, tetrahedron, triangle.  Indices are one exclusive scan over S * 512 counts; no atomics on
 *    global memory, no hashing, no welding: the same input gives the same bits on every run and stream.
 *    Keys.  vert_key (V) i64 = 7 p + slot and face_cell (F) i64 = p of the cell's base, p = (i ny + j) nz + k the dense
 *    linear index.  Sorted by these keys the sparse mesh is section N's mesh of the same volume restricted to the cells of
 *    the cell-active blocks; if every cell with a sign change lies in one, it is section N's mesh, vertex bits and faces.
 *    Need.  need (S) u8, bit o (o in {0,1}^3 as a code) of brick b: some slot owned by a point of b carries a vertex (live,
 *    ends differ) and is also contained in an existing cell of block b - o that is not cell-active.  The surface leaves the
 *    cell-active set exactly there; if no bit is set the mesh is closed wherever the surface does not leave the grid.
 *
 * iso_meshextract_sparse_workspace_bytes: 4 bytes per brick OF THE GRID (the table brick -> list slot, -1 = not listed:
 *   8 MB at 1024^3, 512 MB at 4096^3) plus 17 bytes per listed grid point, the bricks' sums and iso_prefix_sum's
 *   workspace; 0 outside the limits.  16-byte aligned.
 * iso_meshextract_sparse_count: fills the table, pass 1 (one workgroup per listed brick; the 9 x 9 x 9 values its cells
 *   touch are gathered through the table into LDS), need, the totals and the scan.  totals (device, 4 x i64) = vertices,
 *   faces, set need bits over all bricks, bricks whose coords lie outside the grid (such a brick counts nothing).
 *   Enqueues on `stream`, does not synchronise.
 * iso_meshextract_sparse_emit: pass 2 on the workspace the count left, same arguments: verts (V,3) f32, faces (F,3) i32,
 *   and vert_key (V) / face_cell (F) i64 where not NULL.  Reads `totals` back (32 bytes, synchronises the stream): coords
 *   outside the grid and capacities below the totals are ISO_ERR_INVALID; verts / faces may be NULL where the total is 0.
 * Limits: 2 <= nx, ny, nz (ISO_ERR_INVALID below) <= 4096 (ISO_ERR_UNSUPPORTED above); 1 <= S (ISO_ERR_INVALID) and
 *   S * 512 < 2^31 (ISO_ERR_UNSUPPORTED); fewer than 2^31 vertices and fewer than 2^31 faces (ISO_ERR_UNSUPPORTED from
 *   iso_meshextract_sparse_emit).  Unsorted or repeated coords are the caller's to refuse (ops.marching_tetrahedra_bricks
 *   does): the kernels stay in bounds on them, the order of the output is then not the one stated above.           */
int64_t iso_meshextract_sparse_workspace_bytes(int nx, int ny, int nz, int64_t n_bricks);
int iso_meshextract_sparse_count(const float* values, const int32_t* coords, const uint8_t* cell_active, int64_t n_bricks,
                                  int nx, int ny, int nz, float iso, uint8_t* need, int64_t* totals, void* workspace,
                                  int64_t workspace_bytes, void* stream);
int iso_meshextract_sparse_emit(const float* values, const int32_t* coords, const uint8_t* cell_active, int64_t n_bricks,
                                 int nx, int ny, int nz, float ox, float oy, float oz, float sx, float sy, float sz, float iso,
                                 const int64_t* totals, float* verts, int64_t vert_capacity, int32_t* faces,
                                 int64_t face_capacity, int64_t* vert_key, int64_t* face_cell, const void* workspace,
                                 int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISOPOINTS_H_ */
