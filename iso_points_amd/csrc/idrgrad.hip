// Backward of the IDR SDF and of its gradient into every weight and bias and into the points.
// Network (idr.hip): n softplus(beta) layers l = 0 .. n-1 and a linear head l = n.  e = enc(x) (D0 = 3 + 6F entries),
//   in_0 = e, z_l = W_l in_l + b_l, h_l = softplus(z_l), in_(l+1) = h_l, in_skip = [h_(skip-1); e] / sqrt(2),
//   y = w_n . h_(n-1) + b_n, f = tanh(y), g = grad_x f.
// Autograd hands u = dL/df (N) and v = dL/dg (N,3).  With u and v held constant dL/dtheta is the derivative of
// u f + v . g, and v . g is the forward-mode derivative of f along v: ONE tangent column per point (as 3.1c).
//   forward   et_k = dval_k v_c(k) (posenc's dval and coord), int_0 = et, zt_l = W_l int_l, s_l = sigmoid(beta z_l) (1 where
//             beta z_l > 20), ht_l = s_l zt_l, int_skip = [ht_(skip-1); et] / sqrt(2), yt = w_n . ht_(n-1), d = 1 - f^2;
//             the scalar is S = u f + d yt
//   head      ybar = d (u - 2 f yt), ytbar = d, dw_n = sum_p (ybar h_(n-1) + ytbar ht_(n-1)), db_n = sum_p ybar;
//             seeds hbar_(n-1) = ybar w_n, htbar_(n-1) = ytbar w_n
//   reverse   ztbar_l = htbar_l s_l, zbar_l = hbar_l s_l + htbar_l zt_l s'_l, s'_l = beta s_l (1 - s_l) (0 on the linear
//             branch), dW_l = sum_p (zbar_l in_l^T + ztbar_l int_l^T), db_l = sum_p zbar_l,
//             inbar_l = W_l^T zbar_l, intbar_l = W_l^T ztbar_l;  at l = skip both are divided by sqrt(2), the first H - D0
//             entries go on to layer skip-1, the last D0 add into ebar, etbar;  at l = 0 both add into ebar, etbar
//   points    dx_c = sum over k with coord(k) = c of (ebar_k dval_k + etbar_k d2val_k v_c); d2val is 0 for the identity
//             slots, -fr^2 sin for the sine slots, -fr^2 cos for the cosine slots.  No gradient flows into v.
//   v absent  the first-order backward: no tangent column, zbar_l = hbar_l s_l, ybar = d u.
// Kernels (sirengrad.hip's plan; the sweeps share sdf_grad_tile.h, the sums are grad_sums.hip's):
//   sweep     both sweeps of one tile in one workgroup; a wave's 16 matrix-instruction columns are 8 points x {value,
//             tangent} (lane j < 8 the value column of point j, lane j + 8 its tangent column).  Layer 0 multiplies the
//             64-wide padded encoding by FW0 straight from L2 (4 q-chunks: 1 / NT of a hidden layer, no barrier, no second
//             GEMM template in the kernel), the hidden layers are gemm_pass (two chains of H / 2 per
//             output: the chain length decides the distance to float64, mlp_common.h) on FW_l forward and BW_l reverse, layer
//             0's reverse and the encoding Jacobian run on the VALU (W0v) with exact products added in float64.  Stashed:
//             the encoding e | et (64 wide), every in_l | int_l AFTER the concatenation and division (so a hidden dW_l is one
//             product with no special case at the skip layer), and s_l | zt_l s'_l, overwritten in place by zbar_l | ztbar_l.
//             The narrow layer's padded rows are stashed as s = 0 | 0, so their adjoints are exactly zero.
//             Staged layout: 5 * NT * 256 floats of LDS, the whole 160 KiB at NT = 32, as k_idr_step<32> runs.
//                                                                                                  k_idrgrad_sweep<NT, TAN>
//   weights   dW_l = [zbar_l; ztbar_l]^T [in_l; int_l] on the f32 matrix instruction over FIXED chunks of kIgPart points;
//             dW_0 (H x D0) by the same kernel on the 64-wide encoding stash                     k_grad_tn (grad_sums.hip)
//             db_l, dw_n, db_n: column sums in float64 by the same chunks                                   k_idrgrad_cols
//   reduce    the partials added in chunk order, on top of the earlier workspace chunks     k_grad_reduce (grad_sums.hip)
// No float atomic anywhere; a point's dx does not depend on its tile neighbours; the points are taken kIgWs at a time.
#include "grad_sums.h"
#include "idr_common.h"
#include "mfma_split.h"
#include "sdf_grad_tile.h"

namespace {

constexpr int kIgPart = 256;         // points per dW partial (iso_idrgrad_chunk_points)
constexpr int kIgWs = 8192;          // points per workspace chunk (iso_idrgrad_workspace_points): one 32-point tile per CU
constexpr int kIgZeros = 512;        // floats of zeros at the head of the workspace: the tangent columns' "bias"
static_assert(kIgWs % kIgPart == 0, "a workspace chunk holds whole partial chunks");

struct IgArgs {
  const float* pts;                  // (m,3)
  const float* u;                    // (m)
  const float* v;                    // (m,3); unused when TAN is false
  const float* packed;               // iso_idr_pack_weights
  const float* zeros;                // kIgZeros floats of 0
  float* est;                        // rows (R m, kD0Pad): e (and et: row 2p + 1)
  float* ast;                        // in_(l+1) | int_(l+1) at ast + l * lstride, l = 0 .. n-1: rows (R m, H)
  float* sst;                        // the same shape: s_l | zt_l s'_l after the forward sweep, zbar_l | ztbar_l after the reverse
  float* hd;                         // (m,2): ybar, ytbar of the head
  int64_t lstride;
  float* dx;                         // (m,3) or null
  int64_t m;
  IdrShape s;
  float beta;
};

// What slot k's adjoint is multiplied with on its way into dx_coord: dval_k in a value lane, d2val_k v_coord in a tangent lane
__device__ __forceinline__ float ig_enc_jac(int k, float px, float py, float pz, float vx, float vy, float vz, bool tan, int& coord) {
  float val, dv;
  posenc(k, px, py, pz, val, coord, dv);
  if (!tan) return dv;
  if (k < 3) return 0.f;
  const float fr = (float)(1 << ((k - 3) / 6));
  const float vc = coord == 0 ? vx : (coord == 1 ? vy : vz);
  return (-(fr * fr) * val) * vc;
}

template <int NT, bool TAN>
__global__ __launch_bounds__(256, 1) void k_idrgrad_sweep(IgArgs a) {
  constexpr int H = NT * 16;
  constexpr int PW = TAN ? 8 : 16;           // points per wave
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, j = lane & 15;
  const bool tan = TAN && j >= 8;
  float* hL = smem + wave * (NT * 256);
  float* wbuf = smem + 4 * NT * 256;
  f32x4* hL4 = reinterpret_cast<f32x4*>(hL);
  const IdrShape s = a.s;
  const int nL = s.n_layers;
  const int first_enc_slot = H - s.D0;                  // concat: slots [H - D0, H) hold e(x)
  const float sqrt2 = 1.41421356237309515f;             // x / np.sqrt(2) as float32, as k_idr_step divides
  const f32x4* WLimg = reinterpret_cast<const f32x4*>(a.packed + idr_off_wl(H, nL));
  const float b_last = a.packed[idr_off_wl(H, nL) + H];

  const int64_t n_tiles = (a.m + 4 * PW - 1) / (4 * PW);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t p = tile * (4 * PW) + wave * PW + (TAN ? (j & 7) : j);
    const bool valid = p < a.m;
    const int64_t row = TAN ? 2 * p + (tan ? 1 : 0) : p;
    const int64_t roff = row * H + 4 * g;    // + 16 e4: this lane's four features of its stash row
    float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, uu = 0.f;
    if (valid) {
      px = a.pts[p * 3]; py = a.pts[p * 3 + 1]; pz = a.pts[p * 3 + 2];
      uu = a.u[p];
      if constexpr (TAN) {
        if (tan) { vx = a.v[p * 3]; vy = a.v[p * 3 + 1]; vz = a.v[p * 3 + 2]; }
      }
    }
    // ---- encoding -> B operand of layer 0 (slots 16 q + 4 g + i): e in the value lane, et in the tangent lane
#pragma unroll 1
    for (int q = 0; q < kD0Pad / 16; ++q) {
      f32x4 e4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = 16 * q + 4 * g + i;
        float val = 0.f, dv = 0.f; int c = 0;
        if (f < s.D0) posenc(f, px, py, pz, val, c, dv);
        const float vc = c == 0 ? vx : (c == 1 ? vy : vz);
        e4[i] = tan ? dv * vc : val;
      }
      hL4[q * 64 + lane] = e4;
      if (valid) *reinterpret_cast<f32x4*>(a.est + row * kD0Pad + 4 * g + 16 * q) = e4;
    }
    // ---- forward: the tangent columns take a bias of zeros
    f32x4 acc[NT];
    for (int l = 0; l < nL; ++l) {
      if (l == 0) {
        // layer 0: kD0Pad / 16 = 4 q-chunks against the hidden layers' NT -- the A fragments straight from FW0, no LDS stage
        const f32x4* FW0 = reinterpret_cast<const f32x4*>(a.packed + idr_off_fw0(H));
        const float* b0 = tan ? a.zeros : a.packed + idr_off_b0();
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = *reinterpret_cast<const f32x4*>(b0 + 16 * t + 4 * g);
        for (int q = 0; q < kD0Pad / 16; ++q) {
          const f32x4 b4 = hL4[q * 64 + lane];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const f32x4 a4 = FW0[(q * NT + t) * 64 + lane];
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc[t], 0, 0, 0);
          }
        }
      } else {
        const float* base = a.packed + idr_off_layer(H, l);
        gemm_pass<NT, true>(base + H, tan ? a.zeros : base, hL, wbuf, acc, lane, g);
      }
      float* __restrict__ Al = a.ast + (int64_t)l * a.lstride;
      float* __restrict__ Sl = a.sst + (int64_t)l * a.lstride;
      const bool narrow = (s.skip >= 1 && l == s.skip - 1);
#pragma unroll
      for (int t = 0; t < NT; ++t) hL4[t * 64 + lane] = acc[t];
      __builtin_amdgcn_wave_barrier();
#pragma unroll 1
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 own = hL4[e4 * 64 + lane];
        f32x4 zv = own;
        if constexpr (TAN) zv = hL4[e4 * 64 + (lane & ~8)];     // z_l of the point, from its value lane
        __builtin_amdgcn_wave_barrier();
        f32x4 oa, os;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float y, sg, sg2;
          softplus_b2(zv[i], a.beta, y, sg, sg2);
          oa[i] = tan ? sg * own[i] : y;
          os[i] = tan ? own[i] * sg2 : sg;
        }
        if (narrow) {
          // concat [h, e(x)] / sqrt(2): the encoding replaces the zero-padded rows, which keep no derivative at all
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int f = 16 * e4 + 4 * g + i;
            if (f >= first_enc_slot) {
              oa[i] = valid ? a.est[row * kD0Pad + (f - first_enc_slot)] : 0.f;     // e_k / et_k, as stashed above
              os[i] = 0.f;
            }
            oa[i] = oa[i] / sqrt2;
          }
        }
        hL4[e4 * 64 + lane] = oa;
        if (valid) {
          *reinterpret_cast<f32x4*>(Al + roff + 16 * e4) = oa;
          *reinterpret_cast<f32x4*>(Sl + roff + 16 * e4) = os;
        }
      }
    }
    // ---- head: y (value column) and yt (tangent column) in float64, f = tanh(y), d = 1 - f^2
    float scale;
    {
      __builtin_amdgcn_wave_barrier();
      double ys = 0.0;
#pragma unroll 1
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 h4 = hL4[e4 * 64 + lane];
        const f32x4 w4 = WLimg[g * NT + e4];
        ys += ((double)w4.x * (double)h4.x + (double)w4.y * (double)h4.y) + ((double)w4.z * (double)h4.z + (double)w4.w * (double)h4.w);
      }
      ys += __shfl_xor(ys, 16); ys += __shfl_xor(ys, 32);
      double yv = ys, yt = 0.0;
      if constexpr (TAN) {
        const double other = __shfl_xor(ys, 8);
        yv = tan ? other : ys;
        yt = tan ? ys : other;
      }
      const double fd = tanh(yv + (double)b_last);
      const double d = 1.0 - fd * fd;
      const double ybar = d * ((double)uu - 2.0 * fd * yt);
      scale = tan ? (float)d : (float)ybar;
      if (valid && !tan && g == 0) { a.hd[2 * p] = (float)ybar; a.hd[2 * p + 1] = (float)d; }
    }
    // ---- seeds: hbar_(n-1) = ybar w_n in the value lane, htbar_(n-1) = ytbar w_n in the tangent lane
    __builtin_amdgcn_wave_barrier();
    for (int e4 = 0; e4 < NT; ++e4) {
      const f32x4 w4 = WLimg[g * NT + e4];
      hL4[e4 * 64 + lane] = (f32x4){scale * w4.x, scale * w4.y, scale * w4.z, scale * w4.w};
    }
    // ---- reverse; the encoding's adjoints go into dx on the fly, in float64
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (int l = nL - 1; l >= 0; --l) {
      float* Sl = a.sst + (int64_t)l * a.lstride;
      __builtin_amdgcn_wave_barrier();
#pragma unroll 1
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 bar = hL4[e4 * 64 + lane];
        f32x4 barp = bar;
        if constexpr (TAN) barp = hL4[e4 * 64 + (lane ^ 8)];
        __builtin_amdgcn_wave_barrier();
        f32x4 so = {0.f, 0.f, 0.f, 0.f};
        if (valid) so = *reinterpret_cast<const f32x4*>(Sl + roff + 16 * e4);     // s_l (value lane) / zt_l s'_l (tangent lane)
        f32x4 out;
        if constexpr (TAN) {
          f32x4 sp;
#pragma unroll
          for (int i = 0; i < 4; ++i) sp[i] = __shfl_xor(so[i], 8);
#pragma unroll
          for (int i = 0; i < 4; ++i) out[i] = tan ? bar[i] * sp[i] : __builtin_fmaf(bar[i], so[i], barp[i] * sp[i]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) out[i] = bar[i] * so[i];
        }
        hL4[e4 * 64 + lane] = out;
        if (valid) *reinterpret_cast<f32x4*>(Sl + roff + 16 * e4) = out;
      }
      if (l == 0) break;
      const float* base = a.packed + idr_off_layer(H, l);
      sdf_grad_reverse_gemm<NT>(base + H + (int64_t)H * H, hL, wbuf, acc, lane, g);
      if (l == s.skip) {
        // adjoint of [h_(skip-1); e] / sqrt(2): all divided; the encoding slots' part leaves for dx (what stays in those
        // slots meets the narrow layer's stashed zeros)
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int e4 = 0; e4 < NT; ++e4) {
          f32x4 av = hL4[e4 * 64 + lane];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            av[i] = av[i] / sqrt2;
            const int f = 16 * e4 + 4 * g + i;
            if (f >= first_enc_slot) {
              int c;
              const float jac = ig_enc_jac(f - first_enc_slot, px, py, pz, vx, vy, vz, tan, c);
              const double contrib = (double)av[i] * (double)jac;
              gx += c == 0 ? contrib : 0.0;
              gy += c == 1 ? contrib : 0.0;
              gz += c == 2 ? contrib : 0.0;
            }
          }
          hL4[e4 * 64 + lane] = av;
        }
      }
    }
    // ---- layer 0 reverse on the VALU: ebar_k (value lane) / etbar_k (tangent lane) = sum_f W0[f][k] zbar_0[f] over this
    //      lane's features, folded with the encoding Jacobian; exact products added in float64
    if (a.dx) {
      __builtin_amdgcn_wave_barrier();
      const float* W0v = a.packed + idr_off_w0v(H) + (int64_t)g * kW0Row * (H / 4);
#pragma unroll 1
      for (int k = 0; k < s.D0; ++k) {
        const f32x4* col = reinterpret_cast<const f32x4*>(W0v + (int64_t)k * (H / 4));
        double pk = 0.0;
#pragma unroll 1
        for (int e4 = 0; e4 < NT; ++e4) {
          const f32x4 a4 = hL4[e4 * 64 + lane];
          const f32x4 w = col[e4];
          pk += ((double)w.x * (double)a4.x + (double)w.y * (double)a4.y) + ((double)w.z * (double)a4.z + (double)w.w * (double)a4.w);
        }
        int c;
        const float jac = ig_enc_jac(k, px, py, pz, vx, vy, vz, tan, c);
        const double contrib = pk * (double)jac;
        gx += c == 0 ? contrib : 0.0;
        gy += c == 1 ? contrib : 0.0;
        gz += c == 2 ? contrib : 0.0;
      }
      sdf_grad_store_dx<TAN>(gx, gy, gz, a.dx, p, valid && !tan && g == 0);      // the tangent lane holds half the terms
    }
    __syncthreads();
  }
}

template <int NT, bool TAN>
void ig_launch_sweep(const IgArgs& a, hipStream_t st) {
  const int64_t tiles = (a.m + (TAN ? 32 : 64) - 1) / (TAN ? 32 : 64);
  const int blocks = (int)(tiles < kIdrBlocks ? tiles : kIdrBlocks);
  iso_launch_lds<k_idrgrad_sweep<NT, TAN>>(blocks, 256, (size_t)(5 * NT * 256) * sizeof(float), st, a);
}

template <bool TAN>
int ig_dispatch_sweep(const IgArgs& a, int H, hipStream_t st) {
  switch (H / 16) {
    case 8: ig_launch_sweep<8, TAN>(a, st); return 0;
    case 16: ig_launch_sweep<16, TAN>(a, st); return 0;
    case 32: ig_launch_sweep<32, TAN>(a, st); return 0;
    default: return -1;
  }
}

// ---- column sums of one partial chunk: db_l of every softplus layer, dw_n and db_n ---------------------------------------
// The terms are exact products added in float64 and rounded to f32 once.  A workgroup is 64 columns x 4 quarters of the
// chunk's points, the quarters added in order through LDS.  grid (chunks, H / 64, n + 1): z < n is layer z, z = n the head.
struct IgColArgs {
  const float* ast; const float* sst; const float* hd;
  int64_t lstride;
  int R;                             // stash rows per point: 2 in the tangent form
  int64_t m;
  IdrShape s;
  float* part; int64_t part_stride;
};

__global__ __launch_bounds__(256) void k_idrgrad_cols(IgColArgs a) {
  __shared__ double sq[4][2][64];
  const int H = a.s.H, nL = a.s.n_layers, z = blockIdx.z, kq = threadIdx.x & 63, q = threadIdx.x >> 6, k = blockIdx.y * 64 + kq;
  const int R = a.R;
  int64_t p0, pend;
  grad_quarter_range(blockIdx.x, q, kIgPart, a.m, p0, pend);
  double s0 = 0.0, s1 = 0.0;
  if (z < nL) {
    const float* __restrict__ zb = a.sst + (int64_t)z * a.lstride + k;
    for (int64_t p = p0; p < pend; ++p) s0 += (double)zb[R * p * H];
  } else {
    const float* __restrict__ ht = a.ast + (int64_t)(nL - 1) * a.lstride + k;
    for (int64_t p = p0; p < pend; ++p) {
      const double yb = (double)a.hd[2 * p];
      s0 += yb * (double)ht[R * p * H];
      if (R == 2) s0 += (double)a.hd[2 * p + 1] * (double)ht[(2 * p + 1) * H];
      s1 += yb;
    }
  }
  sq[q][0][kq] = s0; sq[q][1][kq] = s1;
  __syncthreads();
  if (q != 0) return;
  const double t0 = (sq[0][0][kq] + sq[1][0][kq]) + (sq[2][0][kq] + sq[3][0][kq]);
  const double t1 = (sq[0][1][kq] + sq[1][1][kq]) + (sq[2][1][kq] + sq[3][1][kq]);
  float* __restrict__ out = a.part + (int64_t)blockIdx.x * a.part_stride;
  if (z < nL) {
    const int od = idr_out_dim(a.s, z);
    if (k < od) out[idr_raw_off(a.s, z) + (int64_t)od * idr_in_dim(a.s, z) + k] = (float)t0;
  } else {
    out[idr_raw_off(a.s, nL) + k] = (float)t0;
    if (k == 0) out[idr_raw_off(a.s, nL) + H] = (float)t1;
  }
}

// workspace (floats) for chunks of mw = min(max(n, 1), kIgWs) points: zeros kIgZeros | encoding stash 2 mw * kD0Pad |
//   in stash n_layers * 2 mw * H | s stash, the same | head mw * 2 | partials ceil(mw / kIgPart) * raw_floats.  Sized for the
//   tangent form; the first-order form uses the first half of every stash.
struct IgWs {
  int64_t mw, zeros, est, ast, sst, hd, part, n_part, raw, lstride, end;
};

IgWs ig_workspace(int64_t n, const IdrShape& s) {
  IgWs w;
  w.mw = n < 1 ? 1 : (n > kIgWs ? kIgWs : n);
  w.raw = idr_raw_off(s, s.n_layers + 1);
  w.n_part = (w.mw + kIgPart - 1) / kIgPart;
  w.lstride = 2 * w.mw * s.H;
  w.zeros = 0;
  w.est = kIgZeros;
  w.ast = w.est + 2 * w.mw * kD0Pad;
  w.sst = w.ast + (int64_t)s.n_layers * w.lstride;
  w.hd = w.sst + (int64_t)s.n_layers * w.lstride;
  w.part = w.hd + 2 * w.mw;
  w.end = w.part + w.n_part * w.raw;
  return w;
}

IdrShape ig_shape(int H, int n_layers, int skip, int F) { return IdrShape{H, n_layers, skip, F, 3 + 6 * F}; }

}  // namespace

// 900 + hidden / 16 for a network the backward runs (every shape the forward entries accept), else 0
extern "C" int iso_idrgrad_form(int hidden, int n_layers, int skip_layer, int n_freq) {
  return idr_shape_ok(hidden, n_layers, skip_layer, n_freq) ? 900 + hidden / 16 : 0;
}

extern "C" int64_t iso_idrgrad_chunk_points() { return kIgPart; }
extern "C" int64_t iso_idrgrad_workspace_points() { return kIgWs; }

extern "C" int64_t iso_idrgrad_workspace_bytes(int64_t n, int hidden, int n_layers, int skip_layer, int n_freq) {
  if (!idr_shape_ok(hidden, n_layers, skip_layer, n_freq)) return 0;
  return 4 * ig_workspace(n, ig_shape(hidden, n_layers, skip_layer, n_freq)).end;
}

extern "C" int iso_idrgrad_backward(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* raw,
                                    const float* packed, int hidden, int n_layers, int skip_layer, int n_freq, float beta,
                                    float* grad_raw_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  (void)raw;
  ISO_REQUIRE(idr_shape_ok(hidden, n_layers, skip_layer, n_freq), ISO_ERR_UNSUPPORTED,
              "iso_idrgrad_backward: unsupported shape (hidden 128/256/512, 2..12 layers, <=10 frequencies)");
  ISO_REQUIRE(beta == 100.0f, ISO_ERR_UNSUPPORTED, "iso_idrgrad_backward: beta must be 100");
  ISO_REQUIRE(n >= 0, ISO_ERR_INVALID, "iso_idrgrad_backward: n < 0");
  const IdrShape s = ig_shape(hidden, n_layers, skip_layer, n_freq);
  const int H = hidden, nL = n_layers;
  hipStream_t st = (hipStream_t)stream;
  const IgWs ws = ig_workspace(n, s);
  if (n == 0) {
    if (grad_raw_out) {
      iso_zero_words(grad_raw_out, ws.raw, st);
      ISO_CHECK_LAUNCH("iso_idrgrad_backward");
    }
    return ISO_OK;
  }
  ISO_REQUIRE(pts && g_sdf && packed && workspace, ISO_ERR_INVALID, "iso_idrgrad_backward: null pointer");
  ISO_REQUIRE(workspace_bytes >= 4 * ws.end, ISO_ERR_WORKSPACE, "iso_idrgrad_backward: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)packed & 15) == 0, ISO_ERR_INVALID,
              "iso_idrgrad_backward: workspace and packed must be 16-byte aligned");
  if (!grad_raw_out && !grad_pts_out) return ISO_OK;

  float* base = (float*)workspace;
  float* part = base + ws.part;
  const int R = g_grad ? 2 : 1;
  iso_zero_words(base + ws.zeros, kIgZeros, st);
  for (int64_t r0 = 0, chunk = 0; r0 < n; r0 += kIgWs, ++chunk) {
    const int64_t m = n - r0 < kIgWs ? n - r0 : kIgWs;
    const int n_part = (int)((m + kIgPart - 1) / kIgPart);
    IgArgs a;
    a.pts = pts + r0 * 3; a.u = g_sdf + r0; a.v = g_grad ? g_grad + r0 * 3 : nullptr;
    a.packed = packed; a.zeros = base + ws.zeros; a.est = base + ws.est; a.ast = base + ws.ast; a.sst = base + ws.sst;
    a.hd = base + ws.hd; a.lstride = ws.lstride;
    a.dx = grad_pts_out ? grad_pts_out + r0 * 3 : nullptr;
    a.m = m; a.s = s; a.beta = beta;
    const int rc = g_grad ? ig_dispatch_sweep<true>(a, H, st) : ig_dispatch_sweep<false>(a, H, st);
    ISO_REQUIRE(rc == 0, ISO_ERR_UNSUPPORTED, "iso_idrgrad_backward: no kernel for hidden size %d", H);
    if (!grad_raw_out) continue;                 // weight gradients not wanted: no partials, no reduce
    for (int l = 0; l < nL; ++l) {
      // zbar_l | ztbar_l against in_l | int_l: the 64-wide encoding stash for layer 0, and the true size of the layer's
      // matrix -- the narrow layer's padded rows and the encoding's padded columns are not written
      GradTnArgs t;
      t.A = a.sst + (int64_t)l * ws.lstride; t.ldA = H;
      t.B = l == 0 ? a.est : a.ast + (int64_t)(l - 1) * ws.lstride; t.ldB = l == 0 ? kD0Pad : H;
      t.rows = R * m; t.rows_per_chunk = (int64_t)R * kIgPart;
      t.part = part + idr_raw_off(s, l); t.part_stride = ws.raw;
      t.out_rows = idr_out_dim(s, l); t.out_cols = idr_in_dim(s, l);
      grad_tn_launch(t, n_part, st);
    }
    IgColArgs c;
    c.ast = a.ast; c.sst = a.sst; c.hd = a.hd; c.lstride = ws.lstride; c.R = R; c.m = m; c.s = s;
    c.part = part; c.part_stride = ws.raw;
    hipLaunchKernelGGL(k_idrgrad_cols, dim3(n_part, H / 64, nL + 1), dim3(256), 0, st, c);
    grad_reduce_launch(part, ws.raw, n_part, ws.raw, chunk > 0, grad_raw_out, st);
  }
  ISO_CHECK_LAUNCH("iso_idrgrad_backward");
  return ISO_OK;
}
