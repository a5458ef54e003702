// Backward of the SIREN SDF and of its gradient into every weight and bias and into the points.
// The forward is  z_0 = W_0 x + b_0, h_0 = sin(w0 z_0), z_l = W_l h_(l-1) + b_l, h_l = sin(wh z_l), f = w_L . h_top + b_L,
// g = grad_x f; autograd hands u = dL/df (n) and v = dL/dg (n,3).  With u and v held constant dL/dtheta is the derivative of
// u f + v . g, and v . g is the forward-mode derivative of f along v: ONE tangent column per point.  s_l = w cos(w z_l):
//   forward   zt_0 = W_0 v, ht_l = s_l zt_l, zt_l = W_l ht_(l-1)
//   head      dw_L = sum_p (u h_top + ht_top), db_L = sum_p u; seeds hbar_top = u w_L, htbar_top = w_L
//   reverse   ztbar_l = htbar_l s_l, zbar_l = hbar_l s_l - w^2 h_l zt_l htbar_l,
//             dW_l = sum_p (zbar_l h_(l-1)^T + ztbar_l ht_(l-1)^T), db_l = sum_p zbar_l,
//             hbar_(l-1) = W_l^T zbar_l, htbar_(l-1) = W_l^T ztbar_l
//   layer 0   dW_0 = sum_p (zbar_0 x^T + ztbar_0 v^T), db_0 = sum_p zbar_0, dx = W_0^T zbar_0 (= u g + Hessian v)
// Kernels:
//   sweep     both sweeps of one tile in one workgroup: a wave's 16 matrix-instruction columns are 8 points x {value,
//             tangent} (lane j < 8 the value column of point j, lane j + 8 its tangent column), so gemm_pass of
//             mlp_common.h runs unchanged on the f32 weight image of iso_siren_pack_weights, FW forward and BW reverse;
//             layer 0 and the seeds on the VALU (z_0, its sine argument and dx in float64: see the sweep's layer 0); every
//             h_l | ht_l and s_l | zt_l stashed, the latter overwritten in place by zbar_l | ztbar_l; dx written
//                                                                                                k_sirengrad_sweep<NT, TAN>
//             TAN = false (v absent): 16 value columns per wave, no tangent, zbar_l = hbar_l s_l
//   weights   dW_l = [zbar_l; ztbar_l]^T [h_(l-1); ht_(l-1)] on the f32 matrix instruction over FIXED chunks of kSgPart
//             points, two accumulation chains (its own kernel for square H x H layers: DESIGN.md 3.1e)    k_sirengrad_tn
//             db_l, dW_0, dw_L, db_L: column sums in float64 by the same chunks                          k_sirengrad_cols
//   reduce    the partials added in chunk order, on top of the earlier workspace chunks  k_grad_reduce (grad_sums.hip)
//   codes     one latent code per cloud: z_0 = W0x x + t_u(p), t_u a row of a table (the sweep's layer 0 takes it per point);
//             dt_u = sum of zbar_0 over the row's points by the same chunks          k_sirencode_rows, k_sirencode_join
// No float atomic anywhere; a point's dx does not depend on its tile neighbours; the points are taken kSgWs at a time.
#include "grad_sums.h"
#include "siren_common.h"
#include "mlp_common.h"
#include "mfma_split.h"
#include "sdf_grad_tile.h"

namespace {

constexpr int kSgPart = 256;         // points per dW partial (iso_sirengrad_chunk_points)
constexpr int kSgWs = 16384;         // points per workspace chunk (iso_sirengrad_workspace_points)
constexpr int kSgBlocks = 512;       // persistent: two workgroups per CU, as k_siren_step
constexpr int kSgZeros = 256;        // floats of zeros at the head of the workspace: the tangent columns' "bias"
static_assert(kSgWs % kSgPart == 0, "a workspace chunk holds whole partial chunks");

bool sg_shape_ok(int H, int L) { return (H == 64 || H == 128 || H == 256) && L >= 0 && L <= 8; }

// raw layout (iso_siren_pack_weights): W0[H*3] b0[H] {Wl[H*H] bl[H]}*L WL[H] bL[1]
__host__ __device__ inline int64_t sg_raw_w(int H, int l) { return l == 0 ? 0 : 4 * (int64_t)H + (int64_t)(l - 1) * ((int64_t)H * H + H); }
__host__ __device__ inline int64_t sg_raw_b(int H, int l) { return l == 0 ? 3 * (int64_t)H : sg_raw_w(H, l) + (int64_t)H * H; }
__host__ __device__ inline int64_t sg_raw_head(int H, int L) { return 4 * (int64_t)H + (int64_t)L * ((int64_t)H * H + H); }
__host__ __device__ inline int64_t sg_raw_floats(int H, int L) { return sg_raw_head(H, L) + H + 1; }

struct SgArgs {
  const float* pts;                  // (m,3)
  const float* u;                    // (m)
  const float* v;                    // (m,3); unused when TAN is false
  const float* packed;               // iso_siren_pack_weights
  const float* zeros;                // kSgZeros floats of 0
  const float* b0_tail;              // (H) or null: layer 0's bias is packed's b_0 + b0_tail, added in float64
  const float* code_bias;            // (n_codes, H) or null: layer 0's bias of point p is row code_of[p] of this table (natural
  const float* code_tail;            //   feature order) + the same row of code_tail (or null), in place of packed's b_0 + b0_tail
  const int32_t* code_of;            // (m) table row of every point, clamped into [0, n_codes) before it addresses anything
  int64_t n_codes;
  float* ast;                        // sine layer l at ast + l * lstride: rows (R m, H), h_l (and ht_l: row 2p + 1)
  float* sst;                        // the same shape: s_l (and zt_l) after the forward sweep, zbar_l (and ztbar_l) after the reverse
  int64_t lstride;
  float* dx;                         // (m,3) or null
  int64_t m;
  int L;
  float w0, wh;
};

template <int NT, bool TAN>
__global__ __launch_bounds__(256, 2) void k_sirengrad_sweep(SgArgs a) {
  constexpr int H = NT * 16;
  constexpr int PW = TAN ? 8 : 16;           // points per wave
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, j = lane & 15;
  const bool tan = TAN && j >= 8;
  float* hL = smem + wave * (NT * 256);
  float* wbuf = smem + 4 * NT * 256;
  const f32x4* W0img = reinterpret_cast<const f32x4*>(a.packed + off_w0(H));
  const f32x4* WLimg = reinterpret_cast<const f32x4*>(a.packed + off_wl(H));
  f32x4* hL4 = reinterpret_cast<f32x4*>(hL);

  const int64_t n_tiles = (a.m + 4 * PW - 1) / (4 * PW);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t p = tile * (4 * PW) + wave * PW + (TAN ? (j & 7) : j);
    const bool valid = p < a.m;
    const int64_t row = TAN ? 2 * p + (tan ? 1 : 0) : p;
    const int64_t roff = row * H + 4 * g;    // + 16 e4: this lane's four features of its stash row
    float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, scale = 0.f;
    if (valid) {
      px = a.pts[p * 3]; py = a.pts[p * 3 + 1]; pz = a.pts[p * 3 + 2];
      scale = a.u[p];
      if constexpr (TAN) {
        if (tan) { vx = a.v[p * 3]; vy = a.v[p * 3 + 1]; vz = a.v[p * 3 + 2]; scale = 1.0f; }
      }
    }
    // ---- layer 0 (3 -> H) on the VALU: the value lane and the tangent lane both form z_0 of their point
    {
      float* __restrict__ A0 = a.ast;
      float* __restrict__ S0 = a.sst;
      // one latent code per cloud (iso_sirencode_backward): the bias is the point's row of a table, a choice made at run
      // time (the same for every lane of a point), so that the instances stay <NT, TAN>
      const bool coded = a.code_bias != nullptr;
      int64_t crow = 4 * g;
      if (coded && valid) {
        int64_t cu = a.code_of[p];
        cu = cu < 0 ? 0 : (cu >= a.n_codes ? a.n_codes - 1 : cu);
        crow += cu * H;
      }
      for (int e4 = 0; e4 < NT; ++e4) {
        f32x4 oa, os;
        f32x4 cb = {0.f, 0.f, 0.f, 0.f}, ct = {0.f, 0.f, 0.f, 0.f};
        if (coded) {
          cb = *reinterpret_cast<const f32x4*>(a.code_bias + crow + 16 * e4);
          if (a.code_tail) ct = *reinterpret_cast<const f32x4*>(a.code_tail + crow + 16 * e4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 w = W0img[g * (H / 4) + e4 * 4 + i];
          // The sine's argument w0 z_0 reaches 30 .. 40: its f32 rounding alone is 1e-6 rad, which every later layer
          // carries on (gain ~1 per layer) and which was the largest single term of the error against float64.  So z_0
          // and the argument are formed in float64 (exact products), cut into an f32 head and tail, and the tail enters
          // through sin(a + t) = sin a + t cos a, cos(a + t) = cos a - t sin a.
          const double b0 = coded ? (double)cb[i] + (double)ct[i]
                                  : (a.b0_tail ? (double)w.w + (double)a.b0_tail[16 * e4 + 4 * g + i] : (double)w.w);
          const double zd = ((double)w.x * (double)px + (double)w.y * (double)py) + ((double)w.z * (double)pz + b0);
          const double ad = (double)a.w0 * zd;
          const float ah = (float)ad, al = (float)(ad - (double)ah);
          float s, c;
          iso_sincos(ah, s, c);
          const float s1 = __builtin_fmaf(c, al, s), c1 = __builtin_fmaf(-s, al, c);
          const float sd = a.w0 * c1;
          const float zt = (float)(((double)w.x * (double)vx + (double)w.y * (double)vy) + (double)w.z * (double)vz);
          oa[i] = tan ? sd * zt : s1;
          os[i] = tan ? zt : sd;
        }
        hL4[e4 * 64 + lane] = oa;
        if (valid) {
          *reinterpret_cast<f32x4*>(A0 + roff + 16 * e4) = oa;
          *reinterpret_cast<f32x4*>(S0 + roff + 16 * e4) = os;
        }
      }
    }
    // ---- hidden layers, forward: the tangent columns take a bias of zeros
    f32x4 acc[NT];
    for (int l = 0; l < a.L; ++l) {
      const float* base = a.packed + off_hidden(H, l);
      gemm_pass<NT, true>(base + H, tan ? a.zeros : base, hL, wbuf, acc, lane, g);
      float* __restrict__ Al = a.ast + (int64_t)(l + 1) * a.lstride;
      float* __restrict__ Sl = a.sst + (int64_t)(l + 1) * a.lstride;
#pragma unroll
      for (int t = 0; t < NT; ++t) hL4[t * 64 + lane] = acc[t];
      __builtin_amdgcn_wave_barrier();
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 own = hL4[e4 * 64 + lane];
        f32x4 zv = own;
        if constexpr (TAN) zv = hL4[e4 * 64 + (lane & ~8)];     // z_l of the point, from its value lane
        __builtin_amdgcn_wave_barrier();
        f32x4 oa, os;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float s, c;
          iso_sincos(a.wh * zv[i], s, c);
          const float sd = a.wh * c;
          oa[i] = tan ? sd * own[i] : s;
          os[i] = tan ? own[i] : sd;
        }
        hL4[e4 * 64 + lane] = oa;
        if (valid) {
          *reinterpret_cast<f32x4*>(Al + roff + 16 * e4) = oa;
          *reinterpret_cast<f32x4*>(Sl + roff + 16 * e4) = os;
        }
      }
    }
    // ---- seeds: hbar_top = u w_L in the value lane, htbar_top = w_L in the tangent lane
    for (int e4 = 0; e4 < NT; ++e4) {
      const f32x4 w4 = WLimg[g * NT + e4];
      hL4[e4 * 64 + lane] = (f32x4){scale * w4.x, scale * w4.y, scale * w4.z, scale * w4.w};
    }
    // ---- reverse
    for (int l = a.L; l >= 0; --l) {
      const float w = l == 0 ? a.w0 : a.wh;
      const float w2 = w * w;
      const float* Al = a.ast + (int64_t)l * a.lstride;
      float* Sl = a.sst + (int64_t)l * a.lstride;
      __builtin_amdgcn_wave_barrier();
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 bar = hL4[e4 * 64 + lane];
        f32x4 barp = bar;
        if constexpr (TAN) barp = hL4[e4 * 64 + (lane ^ 8)];
        __builtin_amdgcn_wave_barrier();
        f32x4 so = {0.f, 0.f, 0.f, 0.f}, h4 = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
          so = *reinterpret_cast<const f32x4*>(Sl + roff + 16 * e4);            // s_l (value lane) / zt_l (tangent lane)
          if (!tan) h4 = *reinterpret_cast<const f32x4*>(Al + roff + 16 * e4);
        }
        f32x4 out;
        if constexpr (TAN) {
          f32x4 sp;
#pragma unroll
          for (int i = 0; i < 4; ++i) sp[i] = __shfl_xor(so[i], 8);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            out[i] = tan ? bar[i] * sp[i] : __builtin_fmaf(bar[i], so[i], -(((w2 * h4[i]) * sp[i]) * barp[i]));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) out[i] = bar[i] * so[i];
        }
        hL4[e4 * 64 + lane] = out;
        if (valid) *reinterpret_cast<f32x4*>(Sl + roff + 16 * e4) = out;
      }
      if (l == 0) break;
      const float* base = a.packed + off_hidden(H, l - 1);
      sdf_grad_reverse_gemm<NT>(base + H + (int64_t)H * H, hL, wbuf, acc, lane, g);
    }
    // ---- dx = W_0^T zbar_0 (the tangent lanes' sums are not used)
    if (a.dx) {
      double gx = 0.0, gy = 0.0, gz = 0.0;     // H exact products per component, added in float64, rounded once
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 a4 = hL4[e4 * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 w = W0img[g * (H / 4) + e4 * 4 + i];
          gx += (double)w.x * (double)a4[i];
          gy += (double)w.y * (double)a4[i];
          gz += (double)w.z * (double)a4[i];
        }
      }
      sdf_grad_store_dx<false>(gx, gy, gz, a.dx, p, valid && !tan && g == 0);
    }
    __syncthreads();
  }
}

template <int NT, bool TAN>
void launch_sweep(const SgArgs& a, hipStream_t st) {
  const int64_t tiles = (a.m + (TAN ? 32 : 64) - 1) / (TAN ? 32 : 64);
  const int blocks = (int)(tiles < kSgBlocks ? tiles : kSgBlocks);
  iso_launch_lds<k_sirengrad_sweep<NT, TAN>>(blocks, 256, (size_t)(5 * NT * 256) * sizeof(float), st, a);
}

template <bool TAN>
int dispatch_sweep(const SgArgs& a, int H, hipStream_t st) {
  switch (H / 16) {
    case 4: launch_sweep<4, TAN>(a, st); return 0;
    case 8: launch_sweep<8, TAN>(a, st); return 0;
    case 16: launch_sweep<16, TAN>(a, st); return 0;
    default: return -1;
  }
}

// ---- dW partial of one hidden layer: part[c][o][i] = sum over the stash rows of chunk c of A[r][o] B[r][i] ----------------
// One wave per 64 x 64 tile of dW, both operands read row-major straight from the stashes, two rows per matrix instruction in
// ascending order (k_texgrad_tn's form, with two chains).  A chunk is `rows_per_chunk` stash rows: kSgPart points, value and
// tangent row.  k_grad_tn of grad_sums.hip is this kernel with a row length per operand and the true size of the matrix as
// arguments; it measured slower here, so the duplicate stays for now.
struct SgTnArgs {
  const float* A;                    // zbar_l | ztbar_l rows (rows, H)
  const float* B;                    // h_(l-1) | ht_(l-1) rows (rows, H)
  int H;
  int64_t rows;
  int64_t rows_per_chunk;
  float* part;                       // partial c at part + c * part_stride
  int64_t part_stride;
};

__global__ __launch_bounds__(256) void k_sirengrad_tn(SgTnArgs a) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int tiles_n = a.H / 64;
  const int tile = blockIdx.x * 4 + w;
  if (tile >= tiles_n * tiles_n) return;             // H = 64: one tile, no barrier below
  const int o0 = 64 * (tile / tiles_n), i0 = 64 * (tile % tiles_n);
  const int64_t ld = a.H;
  const int64_t p0 = (int64_t)blockIdx.y * a.rows_per_chunk;
  const int64_t pend = p0 + a.rows_per_chunk < a.rows ? p0 + a.rows_per_chunk : a.rows;
  // TWO accumulation chains over the rows, the 16-row groups taken alternately, added at the end: a chain is half as long
  // (with a single chain of 512 rows dW_1 of an eight-layer network sat on the float64 margin)
  f32x16 acc[2][2][2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][t][u][r] = 0.f;
  const float* __restrict__ Ap = a.A + o0 + j;
  const float* __restrict__ Bp = a.B + i0 + j;
  auto group = [&](int64_t p, f32x16 (&ac)[2][2]) {      // sixteen rows: 32 loads in flight, then 32 matrix instructions
    float av[8][2], bv[8][2];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t pp = p + 2 * u + hh;
      av[u][0] = Ap[pp * ld]; av[u][1] = Ap[pp * ld + 32];
      bv[u][0] = Bp[pp * ld]; bv[u][1] = Bp[pp * ld + 32];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      ac[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], bv[u][0], ac[0][0], 0, 0, 0);
      ac[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], bv[u][1], ac[0][1], 0, 0, 0);
      ac[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], bv[u][0], ac[1][0], 0, 0, 0);
      ac[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], bv[u][1], ac[1][1], 0, 0, 0);
    }
  };
  int64_t p = p0;
  for (; p + 32 <= pend; p += 32) { group(p, acc[0]); group(p + 16, acc[1]); }
  if (p + 16 <= pend) { group(p, acc[0]); p += 16; }
  for (; p < pend; p += 2) {                   // the last rows, fewer than sixteen, on the second chain
    const int64_t pp = p + hh;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    if (pp < pend) {
      a0 = Ap[pp * ld]; a1 = Ap[pp * ld + 32];
      b0 = Bp[pp * ld]; b1 = Bp[pp * ld + 32];
    }
    acc[1][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[1][0][0], 0, 0, 0);
    acc[1][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1][0][1], 0, 0, 0);
    acc[1][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][1][0], 0, 0, 0);
    acc[1][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1][1], 0, 0, 0);
  }
  float* __restrict__ out = a.part + (int64_t)blockIdx.y * a.part_stride;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = i0 + 32 * u + j;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = o0 + 32 * t + 8 * (r >> 2) + 4 * hh + (r & 3);
        out[(int64_t)row * a.H + col] = acc[0][t][u][r] + acc[1][t][u][r];
      }
    }
}

// ---- column sums of one partial chunk: db_l of every sine layer, dW_0 (H x 3), dw_L and db_L --------------------------------
// The terms are exact products added in float64 and rounded to f32 once (a bias gradient is a sum of terms of both signs:
// f32 chains of a few hundred adds show in it).  A workgroup is 64 columns x 4 quarters of the chunk's points, the quarters
// added in order through LDS.  grid (chunks, H / 64, L + 2): z <= L is sine layer z, z = L + 1 the head.
struct SgColArgs {
  const float* ast; const float* sst;
  int64_t lstride;
  const float* pts; const float* u; const float* v;    // v null: first-order form, one stash row per point
  int64_t m;
  int H, L;
  float* part; int64_t part_stride;
};

__global__ __launch_bounds__(256) void k_sirengrad_cols(SgColArgs a) {
  __shared__ double sq[4][4][64];
  const int H = a.H, z = blockIdx.z, kq = threadIdx.x & 63, q = threadIdx.x >> 6, k = blockIdx.y * 64 + kq;
  const int R = a.v ? 2 : 1;
  int64_t p0, pend;
  grad_quarter_range(blockIdx.x, q, kSgPart, a.m, p0, pend);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (z <= a.L) {
    const float* __restrict__ zb = a.sst + (int64_t)z * a.lstride + k;
    if (z == 0) {
      for (int64_t p = p0; p < pend; ++p) {
        const double zv = (double)zb[R * p * H];
        s[3] += zv;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += zv * (double)a.pts[p * 3 + c];
        if (a.v) {
          const double zt = (double)zb[(2 * p + 1) * H];
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] += zt * (double)a.v[p * 3 + c];
        }
      }
    } else {
      for (int64_t p = p0; p < pend; ++p) s[3] += (double)zb[R * p * H];
    }
  } else {
    const float* __restrict__ ht = a.ast + (int64_t)a.L * a.lstride + k;
    for (int64_t p = p0; p < pend; ++p) {
      const double uu = (double)a.u[p];
      s[0] += uu * (double)ht[R * p * H];
      if (a.v) s[0] += (double)ht[(2 * p + 1) * H];
      s[3] += uu;
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) sq[q][c][kq] = s[c];
  __syncthreads();
  if (q != 0) return;
  double t[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) t[c] = (sq[0][c][kq] + sq[1][c][kq]) + (sq[2][c][kq] + sq[3][c][kq]);
  float* __restrict__ out = a.part + (int64_t)blockIdx.x * a.part_stride;
  if (z <= a.L) {
    out[sg_raw_b(H, z) + k] = (float)t[3];
    if (z == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[(int64_t)k * 3 + c] = (float)t[c];
    }
  } else {
    out[sg_raw_head(H, a.L) + k] = (float)t[0];
    if (k == 0) out[sg_raw_head(H, a.L) + H] = (float)t[3];
  }
}

// ---- dt_u = sum of zbar_0 over the points of code u: the gradient of the table of layer-0 biases (iso_sirencode_backward) ----
// The rows are contiguous: point p of the call belongs to code u iff code_first[u] <= p < code_first[u + 1].  A row is cut at
// the SAME fixed kSgPart-point pieces (and their quarters) as every other sum here, so a long row is spread over the grid
// and its bits depend on the indices alone.  k_sirencode_rows, one workgroup per piece and 64 columns: every thread walks
// its quarter in order, a float64 sum per row it meets; the quarters' first and last sums are joined in order through LDS.
// A row that lies wholly inside the piece without holding its first or its last point is complete and is written to dt; the
// row of the piece's first point and the row of its last go to edge[piece][0 / 1], rounded to f32 once.  k_sirencode_join,
// one thread per entry of dt: the edge partials of the row's pieces in piece order, one float64 chain on top of the earlier
// workspace chunks, as k_grad_reduce; a row with no point in the call gets zeros.  No atomic.
struct ScArgs {
  const float* zb;                   // the value rows of stash layer 0 after the reverse sweep: point p at zb + R p H
  int R, H;
  int64_t m, r0, n;                  // points of this workspace chunk, its first point in the call, points of the call
  const int64_t* code_first;         // (n_codes + 1), every value read is clamped into [0, n]
  int64_t n_codes;
  float* edge;                       // (pieces, 2, H)
  float* dt;                         // (n_codes, H)
  int first_chunk;
};

__device__ __forceinline__ int64_t sc_first(const ScArgs& a, int64_t u) {
  const int64_t f = a.code_first[u];
  return f < 0 ? 0 : (f > a.n ? a.n : f);
}

// the last row in [0, n_codes) that starts at or before point P of the call (rows without points are passed over)
__device__ __forceinline__ int64_t sc_row_of(const ScArgs& a, int64_t P) {
  int64_t lo = 0, hi = a.n_codes - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (sc_first(a, mid) <= P) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// where row u ends, as a point of this workspace chunk; the last row takes whatever is left
__device__ __forceinline__ int64_t sc_end(const ScArgs& a, int64_t u) {
  return u + 1 < a.n_codes ? sc_first(a, u + 1) - a.r0 : INT64_MAX;
}

__global__ __launch_bounds__(256) void k_sirencode_rows(ScArgs a) {
  __shared__ double sq[4][2][64];
  __shared__ int64_t su[4][2];
  const int H = a.H, kq = threadIdx.x & 63, q = threadIdx.x >> 6, k = blockIdx.y * 64 + kq;
  int64_t p0, pend;
  grad_quarter_range(blockIdx.x, q, kSgPart, a.m, p0, pend);
  int64_t u_head = -1, u_tail = -1;
  double s_head = 0.0, s_tail = 0.0;
  if (p0 < pend) {
    const float* __restrict__ zb = a.zb + k;
    int64_t u = sc_row_of(a, a.r0 + p0), next = sc_end(a, u);
    u_head = u;
    bool head = true;
    double s = 0.0;
    for (int64_t p = p0; p < pend; ++p) {
      if (p >= next) {                         // the same for every thread of the wave: a quarter is a wave's
        if (head) { s_head = s; head = false; }
        else a.dt[u * H + k] = (float)s;       // begun and ended inside this quarter: the whole row
        s = 0.0;
        do { ++u; next = sc_end(a, u); } while (p >= next);
      }
      s += (double)zb[a.R * p * H];
    }
    if (head) s_head = s;
    else { u_tail = u; s_tail = s; }
  }
  sq[q][0][kq] = s_head; sq[q][1][kq] = s_tail;
  if (kq == 0) { su[q][0] = u_head; su[q][1] = u_tail; }
  __syncthreads();
  if (q != 0) return;
  const int64_t first = su[0][0];
  int64_t last = first;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (su[i >> 1][i & 1] >= 0) last = su[i >> 1][i & 1];
  float* __restrict__ edge = a.edge + (int64_t)blockIdx.x * 2 * H + k;
  if (first == last) {                         // one row holds the whole piece: k_sirengrad_cols' sum of the quarters
    edge[0] = (float)((sq[0][0][kq] + sq[1][0][kq]) + (sq[2][0][kq] + sq[3][0][kq]));
    edge[H] = 0.f;
    return;
  }
  int64_t cur = first;
  double t = sq[0][0][kq];
  auto close = [&](int64_t row, double sum) {
    if (row == first) edge[0] = (float)sum;
    else if (row == last) edge[H] = (float)sum;
    else a.dt[row * H + k] = (float)sum;       // inside the piece, over a quarter's edge: the whole row
  };
#pragma unroll
  for (int i = 1; i < 8; ++i) {
    const int64_t row = su[i >> 1][i & 1];
    if (row < 0) continue;
    if (row == cur) { t += sq[i >> 1][i & 1][kq]; continue; }
    close(cur, t);
    cur = row; t = sq[i >> 1][i & 1][kq];
  }
  close(cur, t);
}

__global__ __launch_bounds__(256) void k_sirencode_join(ScArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_codes * a.H) return;
  const int64_t u = i / a.H;
  const int k = (int)(i % a.H);
  int64_t ls = sc_first(a, u) - a.r0, le = sc_first(a, u + 1) - a.r0;
  ls = ls < 0 ? 0 : ls;
  le = le > a.m ? a.m : le;
  if (ls >= le) {                              // no point of the row in this workspace chunk
    if (a.first_chunk) a.dt[i] = 0.f;
    return;
  }
  const int64_t c_lo = ls / kSgPart, c_hi = (le - 1) / kSgPart;
  double s = a.first_chunk ? 0.0 : (double)a.dt[i];
  for (int64_t c = c_lo; c <= c_hi; ++c) {
    const int64_t c0 = c * kSgPart, cend = c0 + kSgPart < a.m ? c0 + kSgPart : a.m;
    if (ls <= c0) s += (double)a.edge[(c * 2 + 0) * a.H + k];
    else if (le >= cend) s += (double)a.edge[(c * 2 + 1) * a.H + k];
    else return;                               // wholly inside the piece: k_sirencode_rows wrote the row
  }
  a.dt[i] = (float)s;
}

// workspace (floats) for chunks of mw = min(max(n, 1), kSgWs) points: zeros kSgZeros | h stash (L + 1) * 2 mw * H |
//   s stash, the same | partials ceil(mw / kSgPart) * raw_floats.  Sized for the tangent form; the first-order form uses the
//   first half of every stash layer.
struct SgWs {
  int64_t mw, zeros, ast, sst, part, n_part, raw, lstride, end;
};

SgWs sg_workspace(int64_t n, int H, int L) {
  SgWs w;
  w.mw = n < 1 ? 1 : (n > kSgWs ? kSgWs : n);
  w.raw = sg_raw_floats(H, L);
  w.n_part = (w.mw + kSgPart - 1) / kSgPart;
  w.lstride = 2 * w.mw * H;
  w.zeros = 0;
  w.ast = kSgZeros;
  w.sst = w.ast + (int64_t)(L + 1) * w.lstride;
  w.part = w.sst + (int64_t)(L + 1) * w.lstride;
  w.end = w.part + w.n_part * w.raw;
  return w;
}

// the per-code sum's edge partials, placed after the uncoded layout: two rows of H floats per piece of a workspace chunk
int64_t sc_edge_floats(const SgWs& w, int H) { return w.n_part * 2 * (int64_t)H; }

}  // namespace

// 800 + (padded hidden) / 16 for a network the backward runs -- hidden 1 .. 256 (a width other than 64 / 128 / 256 is
// zero-padded to the next one by the caller), 0 .. 8 hidden layers -- else 0
extern "C" int iso_sirengrad_form(int hidden, int n_hidden) {
  if (hidden < 1 || hidden > 256 || n_hidden < 0 || n_hidden > 8) return 0;
  const int H = hidden <= 64 ? 64 : (hidden <= 128 ? 128 : 256);
  return 800 + H / 16;
}

extern "C" int64_t iso_sirengrad_chunk_points() { return kSgPart; }
extern "C" int64_t iso_sirengrad_workspace_points() { return kSgWs; }

extern "C" int64_t iso_sirengrad_workspace_bytes(int64_t n, int hidden, int n_hidden) {
  if (!sg_shape_ok(hidden, n_hidden)) return 0;
  return 4 * sg_workspace(n, hidden, n_hidden).end;
}

// one latent code per cloud: the table of layer-0 biases and the rows of the points (iso_sirencode_backward)
struct SgCode {
  const float* bias; const float* tail; const int32_t* of; const int64_t* first; int64_t n_codes;
  float* grad_bias_out;
};

// the three entries: `who` names the caller in the error text, `code` null for the uncoded ones
static int sg_backward(const char* who, const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* packed,
                       int hidden, int n_hidden, float omega_first, float omega_hidden, float* grad_raw_out, float* grad_pts_out,
                       void* workspace, int64_t workspace_bytes, void* stream, const float* b0_tail, const SgCode* code) {
  ISO_REQUIRE(sg_shape_ok(hidden, n_hidden), ISO_ERR_UNSUPPORTED,
              "%s: unsupported shape (hidden 64 / 128 / 256, 0..8 hidden layers)", who);
  ISO_REQUIRE(n >= 0, ISO_ERR_INVALID, "%s: n < 0", who);
  ISO_REQUIRE(!code || code->n_codes >= 1, ISO_ERR_INVALID, "%s: n_codes < 1", who);
  const int H = hidden, L = n_hidden;
  hipStream_t st = (hipStream_t)stream;
  const SgWs ws = sg_workspace(n, H, L);
  float* dt = code ? code->grad_bias_out : nullptr;
  if (n == 0) {
    if (grad_raw_out) iso_zero_words(grad_raw_out, ws.raw, st);
    if (dt) iso_zero_words(dt, code->n_codes * H, st);
    if (grad_raw_out || dt) ISO_CHECK_LAUNCH(who);
    return ISO_OK;
  }
  ISO_REQUIRE(pts && g_sdf && packed && workspace, ISO_ERR_INVALID, "%s: null pointer", who);
  ISO_REQUIRE(!code || (code->bias && code->of && code->first), ISO_ERR_INVALID, "%s: null pointer", who);
  ISO_REQUIRE(workspace_bytes >= 4 * (ws.end + (code ? sc_edge_floats(ws, H) : 0)), ISO_ERR_WORKSPACE, "%s: workspace too small",
              who);
  ISO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)packed & 15) == 0, ISO_ERR_INVALID,
              "%s: workspace and packed must be 16-byte aligned", who);
  ISO_REQUIRE(!code || (((uintptr_t)code->bias & 15) == 0 && ((uintptr_t)code->tail & 15) == 0), ISO_ERR_INVALID,
              "%s: code_bias and code_tail must be 16-byte aligned", who);
  if (!grad_raw_out && !grad_pts_out && !dt) return ISO_OK;

  float* base = (float*)workspace;
  float* part = base + ws.part;
  const int R = g_grad ? 2 : 1;
  iso_zero_words(base + ws.zeros, kSgZeros, st);
  for (int64_t r0 = 0, chunk = 0; r0 < n; r0 += kSgWs, ++chunk) {
    const int64_t m = n - r0 < kSgWs ? n - r0 : kSgWs;
    const int n_part = (int)((m + kSgPart - 1) / kSgPart);
    SgArgs a;
    a.pts = pts + r0 * 3; a.u = g_sdf + r0; a.v = g_grad ? g_grad + r0 * 3 : nullptr;
    a.packed = packed; a.b0_tail = b0_tail; a.zeros = base + ws.zeros; a.ast = base + ws.ast; a.sst = base + ws.sst; a.lstride = ws.lstride;
    a.code_bias = code ? code->bias : nullptr; a.code_tail = code ? code->tail : nullptr;
    a.code_of = code ? code->of + r0 : nullptr; a.n_codes = code ? code->n_codes : 0;
    a.dx = grad_pts_out ? grad_pts_out + r0 * 3 : nullptr;
    a.m = m; a.L = L; a.w0 = omega_first; a.wh = omega_hidden;
    const int rc = g_grad ? dispatch_sweep<true>(a, H, st) : dispatch_sweep<false>(a, H, st);
    ISO_REQUIRE(rc == 0, ISO_ERR_UNSUPPORTED, "%s: no kernel for hidden size %d", who, H);
    if (dt) {                                    // the table's gradient: the per-code sums of zbar_0
      ScArgs c;
      c.zb = a.sst; c.R = R; c.H = H; c.m = m; c.r0 = r0; c.n = n; c.code_first = code->first; c.n_codes = code->n_codes;
      c.edge = base + ws.end; c.dt = dt; c.first_chunk = chunk == 0;
      hipLaunchKernelGGL(k_sirencode_rows, dim3(n_part, H / 64), dim3(256), 0, st, c);
      hipLaunchKernelGGL(k_sirencode_join, dim3((unsigned)((code->n_codes * H + 255) / 256)), dim3(256), 0, st, c);
    }
    if (!grad_raw_out) continue;                 // weight gradients not wanted: no partials, no reduce
    const int tiles = (H / 64) * (H / 64);
    for (int l = 1; l <= L; ++l) {
      SgTnArgs t;
      t.A = a.sst + (int64_t)l * ws.lstride; t.B = a.ast + (int64_t)(l - 1) * ws.lstride; t.H = H;
      t.rows = R * m; t.rows_per_chunk = (int64_t)R * kSgPart;
      t.part = part + sg_raw_w(H, l); t.part_stride = ws.raw;
      hipLaunchKernelGGL(k_sirengrad_tn, dim3((tiles + 3) / 4, n_part), dim3(256), 0, st, t);
    }
    SgColArgs c;
    c.ast = a.ast; c.sst = a.sst; c.lstride = ws.lstride; c.pts = a.pts; c.u = a.u; c.v = a.v; c.m = m; c.H = H; c.L = L;
    c.part = part; c.part_stride = ws.raw;
    hipLaunchKernelGGL(k_sirengrad_cols, dim3(n_part, H / 64, L + 2), dim3(256), 0, st, c);
    grad_reduce_launch(part, ws.raw, n_part, ws.raw, chunk > 0, grad_raw_out, st);
  }
  ISO_CHECK_LAUNCH(who);
  return ISO_OK;
}

extern "C" int iso_sirengrad_backward_b0(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* raw,
                                         const float* packed, int hidden, int n_hidden, float omega_first, float omega_hidden,
                                         float* grad_raw_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes,
                                         void* stream, const float* b0_tail) {
  (void)raw;
  return sg_backward("iso_sirengrad_backward", pts, g_sdf, g_grad, n, packed, hidden, n_hidden, omega_first, omega_hidden,
                     grad_raw_out, grad_pts_out, workspace, workspace_bytes, stream, b0_tail, nullptr);
}

extern "C" int iso_sirengrad_backward(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* raw,
                                      const float* packed, int hidden, int n_hidden, float omega_first, float omega_hidden,
                                      float* grad_raw_out, float* grad_pts_out, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  return iso_sirengrad_backward_b0(pts, g_sdf, g_grad, n, raw, packed, hidden, n_hidden, omega_first, omega_hidden, grad_raw_out,
                                   grad_pts_out, workspace, workspace_bytes, stream, nullptr);
}

// ---- one latent code per cloud: layer 0's bias of a point is a row of a table (header: iso_sirencode_backward) -------------
extern "C" int64_t iso_sirencode_workspace_bytes(int64_t n, int hidden, int n_hidden, int64_t n_codes) {
  if (!sg_shape_ok(hidden, n_hidden) || n_codes < 1) return 0;
  const SgWs ws = sg_workspace(n, hidden, n_hidden);
  return 4 * (ws.end + sc_edge_floats(ws, hidden));
}

extern "C" int iso_sirencode_backward(const float* pts, const float* g_sdf, const float* g_grad, int64_t n, const float* packed,
                                      int hidden, int n_hidden, float omega_first, float omega_hidden, const float* code_bias,
                                      const float* code_tail, const int32_t* code_of, const int64_t* code_first, int64_t n_codes,
                                      float* grad_raw_out, float* grad_code_bias_out, float* grad_pts_out, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  const SgCode code = {code_bias, code_tail, code_of, code_first, n_codes, grad_code_bias_out};
  return sg_backward("iso_sirencode_backward", pts, g_sdf, g_grad, n, packed, hidden, n_hidden, omega_first, omega_hidden,
                     grad_raw_out, grad_pts_out, workspace, workspace_bytes, stream, nullptr, &code);
}
