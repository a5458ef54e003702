// Backward of the texture network (texture.hip) into every weight and bias and into codes, normals and points:
//   recompute the forward kernel's own body (tex_forward_tiles of texture_tile.h: row assembly, three-pass split-fp16
//             tex_gemm on the forward's image, per-point scales) without its head; x_0 (m, K0) and every h_l (m, H) stashed
//                                                                                          k_texgrad_fwd_x16<256|512>
//   head      y = W_head h_top + b_head, dy = g (1 - tanh^2 y) / 2, a_top = (W_head^T dy) [h_top > 0]   k_texgrad_head
//   reverse   a_{l-1} = (W_l^T a_l) [h_{l-1} > 0], l = n_layers-1 .. 1, per 64-point tile: tex_gemm on the TRANSPOSED
//             split-fp16 images, the adjoint cut under a per-point scale from the column-sum bound; every a_l stashed
//                                                                                          k_texgrad_rev_x16<256|512>
//   inputs    dx_0 = a_0 W_0 on the f32 matrix instruction, scattered into d codes | d normals | d points; view slots
//             dropped                                                                                 k_texgrad_dx
//   weights   dW_l = a_l^T h_{l-1} on the f32 matrix instruction over FIXED chunks of kTgPart points   k_texgrad_tn
//             db_l, dW_head, db_head by the same chunks                         k_texgrad_bias / k_texgrad_head_partial
//   reduce    the partials added in chunk order, on top of the earlier workspace chunks k_grad_reduce (grad_sums.hip)
// The ReLU mask is torch's (h > 0 <=> z > 0).  A point's rows do not depend on its tile neighbours or on the workgroup that
// drew its tile, no float atomic is used anywhere, and the points are taken kTgWs at a time so that the stashes stay bounded.
// The head adjoint runs between the two tile kernels as a launch of its own.
#include "grad_sums.h"
#include "idr_common.h"
#include "mfma_split.h"
#include "texture_common.h"
#include "texture_tile.h"

namespace {

constexpr int kTgPart = 512;         // points per dW partial (iso_texgrad_chunk_points)
constexpr int kTgWs = 16384;         // points per workspace chunk
static_assert(kTgWs % kTgPart == 0, "a workspace chunk holds whole partial chunks");

// packed_bw (floats): header 64 ([0..7] 2^s_l, [16..23] colsum_l, l >= 1) | head W [3][H] | head b [4] | WT_0 [K0][H] in f32
//   (rows above D0 zero; dx_0 runs on the f32 matrix instruction) | per l = 1..n_layers-1: BW16_l H*H, the split-fp16
//   image of W_l^T in the forward's FW16 layout (texture_gemm.h): output feature = input index i of W_l, K = output index o.
// 2^s_l: max |2^s_l W_l| in [512, 1024), as the forward's; colsum_l = max_i sum_o |W_l[o][i]|, the bound of the reverse sweep
//   |a_{l-1}[i][p]| <= colsum_l max_o |a_l[o][p]|  (mfma_split.h).
constexpr int kTgHdr = 64;
__host__ __device__ inline int tgp_kp(const TexShape& s, int l) { return l == 0 ? s.K0 : s.H; }
__host__ __device__ inline int64_t tgp_head(const TexShape&) { return kTgHdr; }
__host__ __device__ inline int64_t tgp_hbias(const TexShape& s) { return kTgHdr + 3 * (int64_t)s.H; }
__host__ __device__ inline int64_t tgp_wt0(const TexShape& s) { return tgp_hbias(s) + 4; }
__host__ __device__ inline int64_t tgp_bw(const TexShape& s, int l) {      // l >= 1
  return tgp_wt0(s) + (int64_t)s.K0 * s.H + (int64_t)(l - 1) * s.H * s.H;
}
__host__ __device__ inline int64_t tgp_end(const TexShape& s) { return tgp_bw(s, s.n_layers); }

// per layer l >= 1: the weight scale and the largest column sum of |W_l|
__global__ void k_texgrad_stats(const float* __restrict__ raw, float* __restrict__ packed, TexShape s) {
  __shared__ float s_m[256];
  const int H = s.H, l = blockIdx.x;
  float mx = 0.f, cs = 0.f;
  if (l >= 1) {
    const float* __restrict__ Wl = raw + tex_raw_off(s, l);
    for (int i = threadIdx.x; i < H; i += 256) {
      float t = 0.f;
      for (int o = 0; o < H; ++o) { const float u = fabsf(Wl[(int64_t)o * H + i]); t += u; mx = fmaxf(mx, u); }
      cs = fmaxf(cs, t);
    }
  }
  mx = iso_block_max256(mx, s_m); cs = iso_block_max256(cs, s_m);
  if (threadIdx.x == 0) { packed[l] = x3_weight_scale(mx); packed[16 + l] = cs; }
}

__global__ void k_texgrad_pack(const float* __restrict__ raw, float* __restrict__ packed, TexShape s) {
  const int H = s.H, nL = s.n_layers, NTO = H / 32;
  const int64_t HH = (int64_t)H * H;
  const int64_t end = tgp_end(s);
  for (int64_t o = tgp_head(s) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < end; o += (int64_t)gridDim.x * blockDim.x) {
    if (o < tgp_hbias(s)) {
      packed[o] = raw[tex_raw_off(s, nL) + (o - tgp_head(s))];
    } else if (o < tgp_wt0(s)) {
      const int c = (int)(o - tgp_hbias(s));
      packed[o] = c < 3 ? raw[tex_raw_off(s, nL) + 3 * (int64_t)H + c] : 0.f;
    } else if (o < tgp_bw(s, 1)) {
      const int64_t q = o - tgp_wt0(s);
      const int b = (int)(q / H), a = (int)(q % H);            // WT_0[b][a] = W_0[a][b]
      packed[o] = b < s.D0 ? raw[(int64_t)a * s.D0 + b] : 0.f;
    } else {                                                     // fp16 images of W_l^T: one 32-bit word = two halves
      const int64_t r = o - tgp_bw(s, 1);
      const int l = 1 + (int)(r / HH);
      const int64_t q = r % HH;
      const float sc = packed[l];                                // written by k_texgrad_stats, the launch before
      const int d = (int)(q & 3), lane = (int)((q >> 2) & 63);
      const int64_t blk = q >> 8;                                // (ks*NTO + To)*2 + part
      const int part = (int)(blk & 1);
      const int To = (int)((blk >> 1) % NTO), ks = (int)(blk / (2 * NTO));
      const int fo = 32 * To + (lane & 31);                      // output feature of the reverse: input index of W_l
      f32x2 v;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int fi = x3_feat(ks, 8 * (lane >> 5) + 2 * d + u);   // K of the reverse: output index of W_l
        v[u] = raw[tex_raw_off(s, l) + (int64_t)fi * H + fo] * sc;
      }
      reinterpret_cast<unsigned*>(packed)[o] = tex_f16_word(v, part);
    }
  }
}

// ---- out (m, N) = A (m, K) B (N, K)^T, both operands K-contiguous -------------------------------------------------------
// 128 x 64 per workgroup, four waves of 64 x 32 (two accumulators on one B fragment), K in steps of 32 through LDS.
// K and N are multiples of 64 and 32 (the packed image pads them); rows at or above m load zeros and store nothing.

struct TgNtArgs {
  const float* A; int lda;
  const float* B; int ldb;
  int K, N;
  int64_t m;
  float* gcodes; float* gnormals; float* gpoints;     // dx: any may be null
  int C, G, D0;
};

__global__ __launch_bounds__(256) void k_texgrad_dx(TgNtArgs a) {
  constexpr int LP = 33;
  __shared__ float sA[128 * LP];
  __shared__ float sB[64 * LP];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int wm = w & 1, wn = w >> 1;
  const int64_t m0 = (int64_t)blockIdx.x * 128;
  const int n0 = blockIdx.y * 64;
  // FOUR accumulation chains over K, one per 32-wide K-block modulo 4, added pairwise at the end: a chain is K / 4 terms
  // long instead of K (the head bias gradient at codes of 1e3 missed the float64 margin on one chain)
  f32x16 acc[4][2];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][t][r] = 0.f;
  // the next K-block's operands are requested into registers before this block's matrix instructions and written to LDS
  // after them: the global latency rides under 32 matrix instructions per wave
  f32x4 ra[4], rb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, row = idx >> 3, kq = idx & 7;
      const int64_t gm = m0 + row;
      ra[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (gm < a.m) ra[q] = *reinterpret_cast<const f32x4*>(a.A + gm * a.lda + k0 + 4 * kq);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q, row = idx >> 3, kq = idx & 7;
      rb[q] = *reinterpret_cast<const f32x4*>(a.B + (int64_t)(n0 + row) * a.ldb + k0 + 4 * kq);
    }
  };
  auto to_lds = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, row = idx >> 3, kq = idx & 7;
#pragma unroll
      for (int e = 0; e < 4; ++e) sA[row * LP + 4 * kq + e] = ra[q][e];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q, row = idx >> 3, kq = idx & 7;
#pragma unroll
      for (int e = 0; e < 4; ++e) sB[row * LP + 4 * kq + e] = rb[q][e];
    }
  };
  auto mma = [&](f32x16 (&ac)[2]) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float b = sB[(32 * wn + j) * LP + 2 * kk + hh];
      const float a0 = sA[(64 * wm + j) * LP + 2 * kk + hh];
      const float a1 = sA[(64 * wm + 32 + j) * LP + 2 * kk + hh];
      ac[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, ac[0], 0, 0, 0);
      ac[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, ac[1], 0, 0, 0);
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < a.K; k0 += 128) {        // K is uniform: every thread takes the same blocks and barriers
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int kc = k0 + 32 * c;
      if (kc < a.K) {
        to_lds();
        __syncthreads();
        if (kc + 32 < a.K) fetch(kc + 32);
        mma(acc[c]);
        __syncthreads();
      }
    }
  }
  const int col = n0 + 32 * wn + j;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = m0 + 64 * wm + 32 * t + 8 * (r >> 2) + 4 * hh + (r & 3);
      if (row >= a.m) continue;
      const float v = (acc[0][t][r] + acc[1][t][r]) + (acc[2][t][r] + acc[3][t][r]);
      if (col < a.C) { if (a.gcodes) a.gcodes[row * a.C + col] = v; }
      else if (col < a.C + a.G - 3) { if (a.gnormals) a.gnormals[row * 3 + (col - a.C)] = v; }
      else if (col < a.C + a.G) { if (a.gpoints) a.gpoints[row * 3 + (col - (a.C + a.G - 3))] = v; }
    }
}

// ---- head: one wave per point ---------------------------------------------------------------------------------------------
struct TgHeadArgs {
  const float* h_top;                // (m, H)
  const float* w_head;               // [3][H]
  const float* b_head;               // [4]
  const float* grad_rgb;             // (m, 3)
  float* dy;                         // (m, 4)
  float* a_top;                      // (m, H)
  int64_t m;
  int H;
};

__global__ __launch_bounds__(256) void k_texgrad_head(TgHeadArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, H = a.H;
  for (int64_t p = (int64_t)blockIdx.x * 4 + w; p < a.m; p += (int64_t)gridDim.x * 4) {
    const float* __restrict__ hrow = a.h_top + p * H;
    float y[3] = {0.f, 0.f, 0.f};
    for (int k = lane; k < H; k += 64) {
      const float hv = hrow[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) y[c] = __builtin_fmaf(a.w_head[c * H + k], hv, y[c]);
    }
    float dy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = tanhf(iso_wave_sum(y[c]) + a.b_head[c]);
      dy[c] = a.grad_rgb[p * 3 + c] * (1.0f - t * t) * 0.5f;
    }
    if (lane < 3) a.dy[p * 4 + lane] = lane == 0 ? dy[0] : (lane == 1 ? dy[1] : dy[2]);
    if (lane == 3) a.dy[p * 4 + 3] = 0.f;
    for (int k = lane; k < H; k += 64) {
      const float g = __builtin_fmaf(a.w_head[2 * H + k], dy[2], __builtin_fmaf(a.w_head[H + k], dy[1], a.w_head[k] * dy[0]));
      a.a_top[p * H + k] = hrow[k] > 0.f ? g : 0.f;
    }
  }
}

// ---- dW partial of one layer: part[c][o][i] = sum over the points of chunk c of A[p][o] B[p][i] ---------------------------
// One wave per 64 x 64 tile of dW, both operands read row-major straight from the stashes (32 consecutive floats per
// half wave), two points per matrix instruction in ascending order, on ONE accumulation chain (k_grad_tn of grad_sums.hip
// runs two and takes the chunk length as an argument; it measured slower here: DESIGN.md 3.1e).
struct TgTnArgs {
  const float* A; int lda;           // a_l (m, H)
  const float* B; int ldb;           // h_{l-1} (m, H) or x_0 (m, K0)
  int64_t m;
  int n_out;                         // row length of dW_l: H, D0 for layer 0
  int tiles_n;                       // ldb / 64
  float* part;                       // partial c at part + c * part_stride
  int64_t part_stride;
};

__global__ __launch_bounds__(256) void k_texgrad_tn(TgTnArgs a) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int tile = blockIdx.x * 4 + w;
  const int o0 = 64 * (tile / a.tiles_n), i0 = 64 * (tile % a.tiles_n);
  const int64_t p0 = (int64_t)blockIdx.y * kTgPart;
  const int64_t pend = p0 + kTgPart < a.m ? p0 + kTgPart : a.m;
  f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
  const float* __restrict__ Ap = a.A + o0 + j;
  const float* __restrict__ Bp = a.B + i0 + j;
  int64_t p = p0;
  for (; p + 16 <= pend; p += 16) {            // sixteen points: 32 loads in flight, then 32 matrix instructions
    float av[8][2], bv[8][2];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t pp = p + 2 * u + hh;
      av[u][0] = Ap[pp * a.lda]; av[u][1] = Ap[pp * a.lda + 32];
      bv[u][0] = Bp[pp * a.ldb]; bv[u][1] = Bp[pp * a.ldb + 32];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], bv[u][0], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], bv[u][1], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], bv[u][0], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], bv[u][1], acc[1][1], 0, 0, 0);
    }
  }
  for (; p < pend; p += 2) {
    const int64_t pp = p + hh;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    if (pp < pend) {
      a0 = Ap[pp * a.lda]; a1 = Ap[pp * a.lda + 32];
      b0 = Bp[pp * a.ldb]; b1 = Bp[pp * a.ldb + 32];
    }
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
  }
  float* __restrict__ out = a.part + (int64_t)blockIdx.y * a.part_stride;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = i0 + 32 * u + j;
      if (col >= a.n_out) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = o0 + 32 * t + 8 * (r >> 2) + 4 * hh + (r & 3);
        out[(int64_t)row * a.n_out + col] = acc[t][u][r];
      }
    }
}

// Column sums of one partial chunk (db_l, dW_head, db_head).  A bias gradient is a sum of terms of both signs, so its
// largest entry is of the order of sqrt(points) terms and f32 chains of a few hundred adds showed in it (measured: 4.0e-7 of
// the largest entry at 1500 points, torch's pairwise sum 0.7e-7): the terms are added in float64 and rounded to f32 once.
// A workgroup is 64 columns x 4 quarters of the chunk's points (grad_quarter_range); the quarters are added in order through
// LDS.  A quarter's sum runs two float64 chains.
__device__ __forceinline__ double tg_quarter_sum(const float* __restrict__ v, int64_t ld, int64_t p0, int64_t pend) {
  double s0 = 0.0, s1 = 0.0;
  int64_t p = p0;
  for (; p + 2 <= pend; p += 2) { s0 += (double)v[p * ld]; s1 += (double)v[(p + 1) * ld]; }
  if (p < pend) s0 += (double)v[p * ld];
  return s0 + s1;
}

// db_l partial: grid (chunks, H / 64, n_layers)
struct TgBiasArgs {
  const float* ast;                  // layer l at ast + l * layer_stride, (m, H)
  int64_t layer_stride;
  int64_t m;
  float* part; int64_t part_stride;
  TexShape s;
};

__global__ __launch_bounds__(256) void k_texgrad_bias(TgBiasArgs a) {
  __shared__ double sq[4][64];
  const int H = a.s.H, l = blockIdx.z, kq = threadIdx.x & 63, q = threadIdx.x >> 6, k = blockIdx.y * 64 + kq;
  int64_t p0, pend;
  grad_quarter_range(blockIdx.x, q, kTgPart, a.m, p0, pend);
  sq[q][kq] = tg_quarter_sum(a.ast + (int64_t)l * a.layer_stride + k, H, p0, pend);
  __syncthreads();
  if (q == 0)
    a.part[(int64_t)blockIdx.x * a.part_stride + tex_raw_off(a.s, l) + (int64_t)H * tex_in_dim(a.s, l) + k] =
        (float)((sq[0][kq] + sq[1][kq]) + (sq[2][kq] + sq[3][kq]));
}

// dW_head, db_head partial: grid (chunks, H / 64)
struct TgHeadPartArgs {
  const float* h_top; const float* dy;
  int64_t m;
  float* part; int64_t part_stride;
  TexShape s;
};

__global__ __launch_bounds__(256) void k_texgrad_head_partial(TgHeadPartArgs a) {
  __shared__ double sq[4][3][64];
  __shared__ double sb[4][4];
  const int H = a.s.H, kq = threadIdx.x & 63, q = threadIdx.x >> 6, k = blockIdx.y * 64 + kq;
  int64_t p0, pend;
  grad_quarter_range(blockIdx.x, q, kTgPart, a.m, p0, pend);
  // exact products added in float64
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t p = p0; p < pend; ++p) {
    const double h = (double)a.h_top[p * H + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (double)a.dy[p * 4 + c] * h;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) sq[q][c][kq] = s[c];
  if (blockIdx.y == 0 && kq < 3) sb[q][kq] = tg_quarter_sum(a.dy + kq, 4, p0, pend);
  __syncthreads();
  float* __restrict__ out = a.part + (int64_t)blockIdx.x * a.part_stride + tex_raw_off(a.s, a.s.n_layers);
  if (q == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[(int64_t)c * H + k] = (float)((sq[0][c][kq] + sq[1][c][kq]) + (sq[2][c][kq] + sq[3][c][kq]));
    if (blockIdx.y == 0 && kq < 3) out[3 * (int64_t)H + kq] = (float)((sb[0][kq] + sb[1][kq]) + (sb[2][kq] + sb[3][kq]));
  }
}

// ---- recompute: the forward of texture.hip without its head, x_0 and every h_l of a 64-point tile written to the stashes
struct TgFwdArgs {
  TexArgs t;                         // rgb unused
  float* hst;                        // layer l at hst + l * lstride, row-major (n, H)
  int64_t lstride;
  float* x0;                         // (n, K0)
};

template <int H>
__global__ __launch_bounds__(512, 1) void k_texgrad_fwd_x16(TgFwdArgs fa) {
  tex_forward_tiles<H, true>(fa.t, fa.hst, fa.lstride, fa.x0);
}

template <int H>
void launch_texgrad_fwd(const TgFwdArgs& a, hipStream_t st) {
  using S = TexTile<H>;
  iso_launch_lds<k_texgrad_fwd_x16<H>>(iso_capped_grid(a.t.n, S::P, kIdrBlocks), 512, S::kLds, st, a);
}

// ---- reverse sweep: a_{l-1} = (W_l^T a_l) [h_{l-1} > 0] for l = n_layers-1 .. 1 of one 64-point tile, on the tile skeleton of
// the forward (texture_tile.h): its three-pass split-fp16 GEMM on the TRANSPOSED images, acc zeroed instead of the bias.
// The adjoint has no a-priori range: every point carries its own power-of-two scale, taken from the column-sum bound
// colsum_l * max_o |a_l[o][p]| (the maxima ride on the barrier that ends the stage, as the forward's).  a_top comes from
// k_texgrad_head's stash, the mask from the h stash the recompute has just written; every a_l goes to the a stash (the dW
// GEMMs and dx_0 read it).
struct TgRevArgs {
  const float* packed_bw;
  TexShape s;
  int64_t n;
  const float* hst; float* ast;      // layer l at + l * lstride, row-major (n, H)
  int64_t lstride;
  int32_t* tile_ctr;                 // ZERO when the launch starts
};

template <int H>
__global__ __launch_bounds__(512, 1) void k_texgrad_rev_x16(TgRevArgs a) {
  using S = TexTile<H>;
  constexpr int NB = S::NB, TW = S::TW, P = S::P;
  const TexLds<H> c = tex_lds<H>();
  const TexShape s = a.s;
  const int nL = s.n_layers;
  const float* hdr = a.packed_bw;
  auto bw_img = [&](int l) { return tex_wave_img<H>(a.packed_bw + tgp_bw(s, l), c.w); };
  u32x4 A[4][TW];
  tex_prefetch_a<H>(A, bw_img(nL - 1), c.lane);

  float bscale[NB], amax[NB];
  const int64_t count = a.n;
  const int64_t n_tiles = (count + P - 1) / P;
  int64_t next_tile = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile = next_tile) {
    const int drawn = tex_draw_tile(a.tile_ctr);
    f32x16 acc[TW][NB];
    // ---- a_top of the tile into the accumulator registers, its largest entry per point; cut into act once the maxima of
    // all waves give the scale
    {
      const float* __restrict__ at = a.ast + (int64_t)(nL - 1) * a.lstride;
#pragma unroll
      for (int n = 0; n < NB; ++n) amax[n] = 0.f;
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            const int64_t slot = tile * P + 32 * n + c.j;
            f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
            if (slot < count) {
              const float* src = at + slot * H + c.stash_off(t, p);
              lo = *reinterpret_cast<const f32x4*>(src);
              hi = *reinterpret_cast<const f32x4*>(src + 8);
            }
            float m = amax[n];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc[t][n][8 * p + e] = lo[e]; acc[t][n][8 * p + 4 + e] = hi[e];
              m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(lo[e]), __builtin_fabsf(hi[e])));
            }
            amax[n] = m;
          }
    }
    tex_put_amax(c, 0, amax);
    __syncthreads();
    float Mp[NB];
    tex_get_max(c, 0, Mp);
#pragma unroll
    for (int n = 0; n < NB; ++n) bscale[n] = x3_scale_for(Mp[n] * 1.01f);
    tex_requantize<H, true>(c, bscale, amax, true, [&](int t, int p, int n, float (&hv)[8]) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 8; ++e) hv[e] = acc[t][n][8 * p + e];
    });
    __syncthreads();

    int mbuf = 0;
    for (int l = nL - 1; l >= 1; --l) {
      const u32x4* img = bw_img(l);
      const float wsc = hdr[l];
      float zs[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) zs[n] = wsc * bscale[n];
      const bool last = (l == 1);
      const u32x4* nxt = last ? bw_img(nL - 1) : bw_img(l - 1);
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][n][r] = 0.f;
      tex_gemm3<H, false>(c, img, nxt, acc, A);
      __syncthreads();                                   // every wave has read the adjoints
      // column-sum bound of this stage's output per point -> scale of the next operand
      float nscale[NB], iz[NB];
      const float* __restrict__ hm = a.hst + (int64_t)(l - 1) * a.lstride;
      float* __restrict__ al = a.ast + (int64_t)(l - 1) * a.lstride;
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        nscale[n] = last ? 1.0f : x3_scale_for(hdr[16 + l] * Mp[n] * 1.01f);
        iz[n] = 1.0f / zs[n];
      }
      // a_{l-1} = (acc / zs) [h_{l-1} > 0], stashed
      tex_requantize<H, true>(c, nscale, amax, !last, [&](int t, int p, int n, float (&hv)[8]) __attribute__((always_inline)) {
        const int64_t slot = tile * P + 32 * n + c.j;
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = 0.f;
        if (slot < count) {
          const int64_t off = slot * H + c.stash_off(t, p);
          const f32x4 m0 = *reinterpret_cast<const f32x4*>(hm + off);
          const f32x4 m1 = *reinterpret_cast<const f32x4*>(hm + off + 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            hv[e] = m0[e] > 0.f ? acc[t][n][8 * p + e] * iz[n] : 0.f;
            hv[4 + e] = m1[e] > 0.f ? acc[t][n][8 * p + 4 + e] * iz[n] : 0.f;
          }
          tex_store8(al + off, hv);
        }
      });
      if (last) break;
      tex_end_layer(c, mbuf, amax, nscale, bscale, Mp);
    }
    next_tile = tex_next_tile(drawn);
    __syncthreads();
  }
}

template <int H>
void launch_texgrad_rev(const TgRevArgs& a, hipStream_t st) {
  using S = TexTile<H>;
  iso_launch_lds<k_texgrad_rev_x16<H>>(iso_capped_grid(a.n, S::P, kIdrBlocks), 512, S::kLds, st, a);
}

// workspace (floats) for chunks of mw = min(n, kTgWs) points: x_0 mw*K0 | h stash n_layers*mw*H | a stash n_layers*mw*H |
//   dy mw*4 | partials ceil(mw / kTgPart) * raw_floats | tile counter, 64 B
struct TgWs {
  int64_t mw, x0, hst, ast, dy, part, ctr, n_part, raw, end;
};

TgWs tg_workspace(int64_t n, const TexShape& s) {
  TgWs w;
  w.mw = n < 1 ? 1 : (n > kTgWs ? kTgWs : n);
  w.raw = tex_raw_off(s, s.n_layers + 1);
  w.n_part = (w.mw + kTgPart - 1) / kTgPart;
  w.x0 = 0;
  w.hst = w.x0 + w.mw * s.K0;
  w.ast = w.hst + (int64_t)s.n_layers * w.mw * s.H;
  w.dy = w.ast + (int64_t)s.n_layers * w.mw * s.H;
  w.part = w.dy + w.mw * 4;
  w.ctr = w.part + w.n_part * w.raw;
  w.end = w.ctr + 16;
  return w;
}

}  // namespace

// 700 + hidden / 16, one code per width as iso_texture_form's; -1: refused
extern "C" int iso_texgrad_form(int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  return tex_shape_ok(hidden, n_layers, c_dim, geom, n_freq) ? 700 + hidden / 16 : -1;
}

extern "C" int64_t iso_texgrad_packed_floats(int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  if (!tex_shape_ok(hidden, n_layers, c_dim, geom, n_freq)) return 0;
  return tgp_end(tex_shape(hidden, n_layers, c_dim, geom, n_freq));
}

extern "C" int iso_texgrad_pack_weights(const float* raw, float* packed_bw, int hidden, int n_layers, int c_dim, int geom,
                                        int n_freq, void* stream) {
  ISO_REQUIRE(tex_shape_ok(hidden, n_layers, c_dim, geom, n_freq), ISO_ERR_UNSUPPORTED,
              "iso_texgrad_pack_weights: unsupported shape (hidden 256/512, 1..8 layers, c_dim <= 256, geom 3/6, n_freq -1..6)");
  ISO_REQUIRE(raw && packed_bw, ISO_ERR_INVALID, "iso_texgrad_pack_weights: null pointer");
  const TexShape s = tex_shape(hidden, n_layers, c_dim, geom, n_freq);
  hipLaunchKernelGGL(k_texgrad_stats, dim3(n_layers), dim3(256), 0, (hipStream_t)stream, raw, packed_bw, s);
  hipLaunchKernelGGL(k_texgrad_pack, dim3(iso_stream_grid(tgp_end(s), 256)), dim3(256), 0, (hipStream_t)stream, raw, packed_bw, s);
  ISO_CHECK_LAUNCH("iso_texgrad_pack_weights");
  return ISO_OK;
}

extern "C" int64_t iso_texgrad_chunk_points() { return kTgPart; }
extern "C" int64_t iso_texgrad_workspace_points() { return kTgWs; }

extern "C" int64_t iso_texgrad_workspace_bytes(int64_t n, int hidden, int n_layers, int c_dim, int geom, int n_freq) {
  if (!tex_shape_ok(hidden, n_layers, c_dim, geom, n_freq)) return 0;
  return 4 * tg_workspace(n, tex_shape(hidden, n_layers, c_dim, geom, n_freq)).end;
}

extern "C" int iso_texgrad_backward(const float* points, const float* normals, const float* codes, const float* view_origins,
                                    const int32_t* origin_of, int64_t n_origins, const float* grad_rgb, int64_t n,
                                    const float* packed_fw, const float* packed_bw, int hidden, int n_layers, int c_dim, int geom, int n_freq,
                                    float* grad_raw_out, float* grad_points, float* grad_normals, float* grad_codes,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "iso_texgrad_backward";
  if (int rc = tex_check_shape(fn, n, hidden, n_layers, c_dim, geom, n_freq)) return rc;
  const TexShape s = tex_shape(hidden, n_layers, c_dim, geom, n_freq);
  hipStream_t st = (hipStream_t)stream;
  const TgWs ws = tg_workspace(n, s);
  if (n == 0) {
    if (grad_raw_out) iso_zero_words(grad_raw_out, ws.raw, st);
    ISO_CHECK_LAUNCH("iso_texgrad_backward");
    return ISO_OK;
  }
  if (int rc = tex_check_inputs(fn, points && grad_rgb && packed_fw && packed_bw && workspace, normals, codes, view_origins,
                                origin_of, n_origins, c_dim, geom, n_freq))
    return rc;
  ISO_REQUIRE(geom == 6 || !grad_normals, ISO_ERR_INVALID, "iso_texgrad_backward: grad_normals without normals");
  ISO_REQUIRE(c_dim > 0 || !grad_codes, ISO_ERR_INVALID, "iso_texgrad_backward: grad_codes without codes");
  ISO_REQUIRE(workspace_bytes >= 4 * ws.end, ISO_ERR_INVALID, "iso_texgrad_backward: workspace too small");
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)packed_fw & 15) == 0 && ((uintptr_t)packed_bw & 15) == 0,
              ISO_ERR_INVALID, "iso_texgrad_backward: workspace, packed_fw and packed_bw must be 16-byte aligned");

  const int H = s.H, nL = s.n_layers;
  float* base = (float*)workspace;
  float* x0 = base + ws.x0;
  float* dy = base + ws.dy;
  float* part = base + ws.part;
  const int64_t lstride = ws.mw * H;
  auto hst = [&](int l) { return base + ws.hst + l * lstride; };
  auto ast = [&](int l) { return base + ws.ast + l * lstride; };
  const bool want_dx = grad_points || grad_normals || grad_codes;

  for (int64_t r0 = 0, chunk = 0; r0 < n; r0 += kTgWs, ++chunk) {
    const int64_t m = n - r0 < kTgWs ? n - r0 : kTgWs;
    const int n_part = (int)((m + kTgPart - 1) / kTgPart);
    const int gm = (int)((m + 127) / 128);
    // recompute
    TgFwdArgs fw;
    fw.t.points = points + r0 * 3; fw.t.normals = normals ? normals + r0 * 3 : nullptr;
    fw.t.codes = codes ? codes + r0 * s.C : nullptr; fw.t.origins = view_origins;
    fw.t.origin_of = origin_of ? origin_of + r0 : nullptr; fw.t.n_origins = n_origins; fw.t.rgb = nullptr; fw.t.n = m; fw.t.packed = packed_fw;
    fw.t.s = s; fw.t.tile_ctr = (int32_t*)(base + ws.ctr);
    fw.hst = hst(0); fw.lstride = lstride; fw.x0 = x0;
    iso_zero_words(base + ws.ctr, 1, st);
    if (H == 256) launch_texgrad_fwd<256>(fw, st);
    else launch_texgrad_fwd<512>(fw, st);
    // head
    TgHeadArgs ha;
    ha.h_top = hst(nL - 1); ha.w_head = packed_bw + tgp_head(s); ha.b_head = packed_bw + tgp_hbias(s);
    ha.grad_rgb = grad_rgb + r0 * 3; ha.dy = dy; ha.a_top = ast(nL - 1); ha.m = m; ha.H = H;
    hipLaunchKernelGGL(k_texgrad_head, dim3(iso_capped_grid(m, 4, 4096)), dim3(256), 0, st, ha);
    // reverse
    if (nL > 1) {
      TgRevArgs rv;
      rv.packed_bw = packed_bw; rv.s = s; rv.n = m; rv.hst = hst(0); rv.ast = ast(0); rv.lstride = lstride;
      rv.tile_ctr = (int32_t*)(base + ws.ctr);
      iso_zero_words(base + ws.ctr, 1, st);
      if (H == 256) launch_texgrad_rev<256>(rv, st);
      else launch_texgrad_rev<512>(rv, st);
    }
    if (want_dx) {
      TgNtArgs g = {};
      g.A = ast(0); g.lda = H; g.B = packed_bw + tgp_wt0(s); g.ldb = H; g.K = H; g.N = s.K0; g.m = m;
      g.gcodes = grad_codes ? grad_codes + r0 * s.C : nullptr;
      g.gnormals = grad_normals ? grad_normals + r0 * 3 : nullptr;
      g.gpoints = grad_points ? grad_points + r0 * 3 : nullptr;
      g.C = s.C; g.G = s.G; g.D0 = s.D0;
      hipLaunchKernelGGL(k_texgrad_dx, dim3(gm, s.K0 / 64), dim3(256), 0, st, g);
    }
    if (!grad_raw_out) continue;                 // weight gradients not wanted: no partials, no reduce
    // weight partials
    for (int l = 0; l < nL; ++l) {
      TgTnArgs t;
      t.A = ast(l); t.lda = H; t.B = l == 0 ? x0 : hst(l - 1); t.ldb = tgp_kp(s, l); t.m = m;
      t.n_out = tex_in_dim(s, l); t.tiles_n = tgp_kp(s, l) / 64;
      t.part = part + tex_raw_off(s, l); t.part_stride = ws.raw;
      hipLaunchKernelGGL(k_texgrad_tn, dim3((H / 64) * t.tiles_n / 4, n_part), dim3(256), 0, st, t);
    }
    TgBiasArgs ba;
    ba.ast = ast(0); ba.layer_stride = lstride; ba.m = m; ba.part = part; ba.part_stride = ws.raw; ba.s = s;
    hipLaunchKernelGGL(k_texgrad_bias, dim3(n_part, H / 64, nL), dim3(256), 0, st, ba);
    TgHeadPartArgs hp;
    hp.h_top = hst(nL - 1); hp.dy = dy; hp.m = m; hp.part = part; hp.part_stride = ws.raw; hp.s = s;
    hipLaunchKernelGGL(k_texgrad_head_partial, dim3(n_part, H / 64), dim3(256), 0, st, hp);
    grad_reduce_launch(part, ws.raw, n_part, ws.raw, chunk > 0, grad_raw_out, st);
  }
  ISO_CHECK_LAUNCH("iso_texgrad_backward");
  return ISO_OK;
}
