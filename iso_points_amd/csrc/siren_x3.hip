// Fused SIREN SDF + gradient evaluation and Newton step with the hidden-layer GEMMs on the
// 16-bit matrix cores at f32 accuracy (v_mfma_f32_32x32x16_f16 / _bf16, gfx950).
//
// Reference semantics are those of siren_f32.hip (Siren.forward DSS/models/common.py:140-165 under
// autograd.grad in UniformProjection._compute_sdf_and_grad, levelset_sampling.py:142-170, iterated
// by _project_points :313-342); this file only changes how the H x H products are formed.
//
// f32 product from 16-bit MFMAs (mfma_split.h): every f32
// operand is cut into TWO fp16 numbers (11 + 11 significant bits, round-to-nearest at each cut:
// <= 2^-22 relative in the worst case) under an exact power-of-two scale -- per layer for the weights, 2^12 for
// the activations, per point for the adjoint of the reverse sweep -- and W.x is accumulated in f32
// from three products  Wl.xh + Wh.xl + Wh.xh  (fp16 x fp16 is exact in f32; the dropped Wl.xl is
// <= 2^-22 relative; see mfma_split.h for what that means against the 2^-24 of f32).  The fp16 pipe runs 16x the f32 MFMA rate, so three passes are 5.3x faster than
// one f32 pass; measured against float64 in tests/test_projection_gpu.py next to the f32-MFMA
// kernel.  (The file started with an exact three-way bf16 cut, six products -- hence the x3 in the names; that
// form and the overlap experiments built on it are in tools/experiments/ and in the history.)
//
// Work decomposition (differs from siren_f32.hip: weights are NOT staged through LDS)
//   * one workgroup = P = 32*NB points (NB = 3), NW = 8 waves (two per SIMD; NW = 4 also builds).
//   * the OUTPUT features of a layer are split across the waves (wave w owns tiles
//     TW*w .. TW*w+TW-1 of 32 features): each weight element is needed by exactly one wave,
//     which streams it from L2 straight into registers (lane-linear pre-split image, one 16-B
//     load per lane per (K-step, tile, part)), three K-steps ahead through four rotating register
//     sets that run on across layers and tiles; with 8 waves the operand requests are pinned one
//     behind each of the first MFMAs of a K-step (gemm_x3).
//   * the activations of all P points live in LDS, already split (2 x 8 fp16 per lane entry,
//     [K-step][point tile][part][lane]: every B operand is one conflict-free ds_read_b128).
//     Each wave reads all of them, and after the GEMM writes the K-steps made of its own output
//     features.  Two workgroup barriers per layer (readers done / writers done) replace the
//     per-chunk staging barriers of the f32 kernel.
//   * sin/cos: software reduction to [-1/2, 1/2] revolutions on packed f32 ops, then v_sin_f32 /
//     v_cos_f32 (mlp_common.h); a lane walks its accumulators with static indices, eight values at a
//     time (shapes with more than 8 groups per lane park them in LDS first).
//   * reverse sweep: same GEMM on the transposed image; w*cos(w z) comes back from the
//     per-lane global stash (written in the forward sweep by the same lane).
//   * the on-chip form (x3_step_body with LT > 0; iso_siren_set_step_form, the default for H = 256 with two or three
//     hidden layers): four waves, one per SIMD with 512 registers, two output tiles each; the layers are expanded at
//     compile time and the stash is LDS + a register array -- nothing of it leaves the CU.  Bit-identical results.
#include <stdlib.h>
#include <type_traits>
#include "siren_common.h"
#include "iso_newton.h"
#include "mlp_common.h"

#include "mfma_split.h"

// weight fragments requested three K-steps ahead (gemm_x3): an L2 hit under load takes longer than one K-step of MFMAs
constexpr int kAD = 3;

namespace {

// s = sin(w_in * z), c = w * cos(w_in * z); w_in = w / (accumulator scale), an exact power-of-two quotient
__device__ __forceinline__ void x3_sin_wcos8(float w_in, float w, const float (&z)[8], float (&s)[8], float (&c)[8]) {
  iso_sin_wcos8(w_in, w, z, s, c);
}


// ---- packing -------------------------------------------------------------------------------
// raw layout: W0[H*3] b0[H] {Wi[H*H] bi[H]}*L WL[H] bL[1]
// the K-order vectors: W0k, WLk, the biases of the hidden layers
__global__ void k_siren_pack_x3(const float* __restrict__ raw, float* __restrict__ packed, int H, int L) {
  const int64_t base = x3_base(H, L), total = x16_base(H, L);
  const int64_t HH = (int64_t)H * H;
  const float* b0 = raw + (int64_t)H * 3;
  const float* WL = raw + (int64_t)H * 4 + (int64_t)L * (HH + H);
  for (int64_t o = base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t rel = o - base;
    auto feat_of = [](int64_t ko) { return x3_feat((int)(ko >> 4), 8 * (int)((ko >> 3) & 1) + (int)(ko & 7)); };
    if (rel < 4 * (int64_t)H) {
      const int f = feat_of(rel >> 2), c = (int)(rel & 3);
      packed[o] = (c < 3) ? raw[f * 3 + c] : b0[f];
    } else if (rel < 5 * (int64_t)H) {
      packed[o] = WL[feat_of(rel - 4 * (int64_t)H)];
    } else {
      const int64_t r2 = rel - 5 * (int64_t)H;          // bias of hidden layer l, K-order
      const int l = (int)(r2 / H);
      const float* Wl = raw + (int64_t)H * 4 + (int64_t)l * (HH + H);
      packed[o] = Wl[HH + feat_of(r2 % H)];
    }
  }
}

// power-of-two scale of every hidden layer: max |2^s W| in [512, 1024)
__global__ void k_siren_wscale(const float* __restrict__ raw, float* __restrict__ packed, int H, int L) {
  __shared__ float s_m[256];
  const int l = blockIdx.x;
  const int64_t HH = (int64_t)H * H;
  const float* Wl = raw + (int64_t)H * 4 + (int64_t)l * (HH + H);
  // ONE pass over the layer (column f of thread f, rows in order: coalesced across the workgroup, 32 loads in flight --
  // the loop is a latency chain otherwise): the maximum for the scale and the column sums for c_l below.  (Two passes
  // with 16 loads in flight were 17 us per cycle; the weights change every step, so this runs every cycle.)
  float m = 0.f, cs = 0.f;
  for (int f = threadIdx.x; f < H; f += 256) {
    float t = 0.f;
#pragma unroll 32
    for (int k = 0; k < H; ++k) {
      const float a = fabsf(Wl[(int64_t)k * H + f]);
      m = (a == a && a > m) ? a : m;
      t += a;
    }
    cs = fmaxf(cs, t);
  }
  s_m[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_m[threadIdx.x] = fmaxf(s_m[threadIdx.x], s_m[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    packed[x16_base(H, L) + l] = x3_weight_scale(s_m[0]);
  }
  __syncthreads();
  // c_l = max_f sum_k |W_l[k][f]|: |(W_l^T a)[f]| <= c_l max|a|
  s_m[threadIdx.x] = cs;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_m[threadIdx.x] = fmaxf(s_m[threadIdx.x], s_m[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) packed[x16_base(H, L) + 8 + l] = s_m[0];
  if (l == 0) {
    __syncthreads();
    const float* WLh = raw + (int64_t)H * 4 + (int64_t)L * (HH + H);
    float mh = 0.f;
    for (int f = threadIdx.x; f < H; f += 256) mh = fmaxf(mh, fabsf(WLh[f]));
    s_m[threadIdx.x] = mh;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) s_m[threadIdx.x] = fmaxf(s_m[threadIdx.x], s_m[threadIdx.x + o]);
      __syncthreads();
    }
    if (threadIdx.x == 0) packed[x16_base(H, L) + 16] = s_m[0];
  }
}

__global__ void k_siren_pack_f16(const float* __restrict__ raw, float* __restrict__ packed, int H, int L) {
  const int64_t HH = (int64_t)H * H;
  const int NTO = H / 32;
  const int64_t total = 2 * (int64_t)L * HH;       // forward images, then transposed ones
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const bool bwd = o >= (int64_t)L * HH;
    const int l = (int)((o / HH) % L);
    const int64_t q = o % HH;
    const float* Wl = raw + (int64_t)H * 4 + (int64_t)l * (HH + H);
    const float sc = packed[x16_base(H, L) + l];
    const int d = (int)(q & 3), lane = (int)((q >> 2) & 63);
    const int64_t blk = q >> 8;                 // (s*NTO + To)*2 + part
    const int part = (int)(blk & 1);
    const int To = (int)((blk >> 1) % NTO), s = (int)(blk / (2 * NTO));
    const int fo = 32 * To + (lane & 31);
    f32x2 v;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int fi = x3_feat(s, 8 * (lane >> 5) + 2 * d + u);
      v[u] = (bwd ? Wl[(int64_t)fi * H + fo] : Wl[(int64_t)fo * H + fi]) * sc;
    }
    const f16x2 h = __builtin_convertvector(v, f16x2);
    const f16x2 lo = __builtin_convertvector(v - __builtin_convertvector(h, f32x2), f16x2);
    reinterpret_cast<unsigned*>(packed + x16_off_layer(H, L, 0))[o] =
        part == 0 ? __builtin_bit_cast(unsigned, h) : __builtin_bit_cast(unsigned, lo);
  }
}

// ---- the step kernel -------------------------------------------------------------------------
// RP: head / gradient partial sums a wave hands to the final reduction.  RP > 1 is the on-chip form of four waves: one
// partial per 32-feature output tile, as the eight-wave form has them; there the `red` region holds the exchange of the
// adjoint maxima only, and the final reduction goes through the LDS part of the stash, which is dead by then.
template <int H, int NW, int NB, int RP = 1>
struct X3Shape {
  static constexpr int NS = H / 16;        // K-steps of a hidden layer
  static constexpr int NTO = H / 32;       // output tiles
  static constexpr int TW = NTO / NW;      // output tiles per wave
  static constexpr int SL = 2 * TW;        // K-steps of the next layer produced by one wave
  static constexpr int NG = SL * NB;       // 8-value groups per lane
  static constexpr int P = 32 * NB;        // points per workgroup
  static constexpr size_t kActBytes = (size_t)NS * NB * kAP * 1024;
  static constexpr size_t kRedBytes = RP > 1 ? (size_t)2 * P * NW * 4 : (size_t)NW * P * 16;
  static constexpr size_t kPtsBytes = (size_t)P * 16;                 // the tile's points, for the reverse sweep's layer 0
  // LDS-resident part of the derivative stash: the first LG of the NG groups per lane of stash slot 0 (written by
  // hidden layer 0, read back last of all by reverse stage 1 -- the longest-lived slot) stay in the CU; 2 KiB per
  // group and wave, as many groups as the 160 KiB of a gfx950 CU leave room for
  static constexpr int kLdsGroupsFit = (int)((163840 - (kActBytes + kRedBytes + kPtsBytes)) / ((size_t)NW * 2048));
  static constexpr int LG = kLdsGroupsFit < NG ? kLdsGroupsFit : NG;
  static constexpr size_t kLds = kActBytes + kRedBytes + kPtsBytes + (size_t)NW * LG * 2048;
  // slot l of the global stash = w cos(w z) of hidden layer l's output (layer 0's is recomputed, the top layer's is
  // consumed on the spot): L - 1 slots in use, one kept for L = 1
  static constexpr int64_t kStashPerWg(int L) { return (int64_t)NW * (L > 1 ? L : 1) * NG * 512; }  // floats
  static_assert(NTO % NW == 0 && TW >= 1, "features must split evenly over the waves");
  static_assert(RP == 1 || (size_t)NW * LG * 2048 >= (size_t)NW * RP * P * 16, "the final reduction fits the LDS stash");
};

// the layer-0 biases of K-step s for lane half h (features x3_feat(s, 8h + e), e = 0..7: 16 s + 8 (e >> 2) + 4h + (e & 3))
// from row `row` of the per-code table: two aligned 16-B loads
template <int H>
__device__ __forceinline__ void x3_code_bias8(const float* table, int row, int s, int h, float (&b)[8]) {
  const f32x4* t = reinterpret_cast<const f32x4*>(table + (int64_t)row * H + 16 * s + 4 * h);
  const f32x4 lo = t[0], hi = t[2];
#pragma unroll
  for (int e = 0; e < 4; ++e) { b[e] = lo[e]; b[4 + e] = hi[e]; }
}

// FWD: value only (iso_siren_sdf, sphere tracing) -- no stash, no reverse sweep, no w cos(w z)
// bid / nblk: this workgroup's index among the nblk workgroups that share the list (the kernels below)
// sid: index of the workgroup's stash region (= bid unless the caller runs private lists, see k_siren_tail_x3)
// CODED: layer 0's bias is row code_of[idx] of the per-code table a.code_bias (SirenCodedArgs, natural feature order) instead of
// the .w slot of the W0 image, in the forward sweep and where reverse stage 0 forms z0 again; the expression is the same,
// so a coded evaluation equals the uncoded one of the network whose b0 is that row, bit for bit
// LT > 0: the ON-CHIP form (iso_siren_set_step_form; gradient kernels of LT hidden layers, a.L == LT).  The layer loops
// are expanded with the layer a compile-time constant, so every stash index is static and the part of the derivative
// stash that does not fit LDS is a register array from the forward activation that writes it to the reverse stage that
// reads it: no global stash access.  Built for four waves (one per SIMD, 512 registers each): a wave owns TW = 2 output
// tiles and keeps the head / gradient partial sums of each apart (RP = TW), accumulated in the order the eight-wave
// form uses for the wave that owns that tile alone, so the final reduction adds the same eight numbers in the same
// order and a point's result is that of the eight-wave form bit for bit.
template <int H, int NW, int NB, bool FWD, bool CODED, int LT = 0>
__device__ __forceinline__ void x3_step_body(const typename SirenArgsOf<CODED>::type& a, const int bid, const int nblk,
                                             const int sid) {
  constexpr bool RS = LT > 0;                        // register stash
  constexpr int RP = RS ? (H / 32) / NW : 1;
  static_assert(!RS || !FWD, "the on-chip form is a gradient kernel");
  using S = X3Shape<H, NW, NB, RP>;
  constexpr int NS = S::NS, NTO = S::NTO, TW = S::TW, SL = S::SL, NG = S::NG, P = S::P;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32x4* act = reinterpret_cast<u32x4*>(smem_raw);
  f32x4* red = reinterpret_cast<f32x4*>(smem_raw + S::kActBytes);   // [NW][P] {f,gx,gy,gz}
  f32x4* ptl = reinterpret_cast<f32x4*>(smem_raw + S::kActBytes + S::kRedBytes);                  // [P] {x,y,z,-}
  constexpr int LG = S::LG;
  const int tid = threadIdx.x;
  // the wave index is wave-uniform: say so, and everything derived from it (weight-image and
  // stash bases) lives in SGPRs; loads then use the scalar-base + lane-offset form
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, h = lane >> 5, j = lane & 31;
  u32x4* own = act + (size_t)(SL * w) * NB * kAP * 64 + lane;    // this wave's K-steps (+lane)
  u32x4* park = own + (size_t)(kAP - 2) * NG * 64;               // last NG*2 KiB of the region
  // Operand loads pinned behind the MFMAs (gemm_x3): used for the 8-wave shape only.  The 4-wave,
  // two-workgroups-per-CU build of H = 128 loses run-to-run repeatability as soon as the loads may
  // be scheduled between the MFMAs (tools/siren_stress.py: every repeat differs; the same source
  // with one workgroup per CU, and the 8-wave H = 256 build over 60 chaotic-weight repeats, are
  // bit-stable).  Cause not found yet, so that shape keeps the loads in front of the MFMA block.
  constexpr bool IL = (NW == 8) || RS;     // (RS: one workgroup per CU)
  const int L = RS ? LT : a.L;
  const float* X = a.packed + x3_base(H, L);
  // wave-uniform bases (SGPRs) + small per-lane offsets: no 64-bit per-lane pointers are kept live
  const f32x4* W0u = reinterpret_cast<const f32x4*>(X) + SL * w * 16;       // + h*8 + ...
  const float* WLu = X + 4 * H + SL * w * 16;                               // + h*8 + ...
  const int h8 = h * 8;
  const float bL = a.packed[off_bl(H)];
  f32x4* stash = reinterpret_cast<f32x4*>(a.stash) +
                 ((int64_t)sid * NW + w) * (int64_t)(L > 1 ? L : 1) * NG * 128;   // + lane
  f32x4* lst = reinterpret_cast<f32x4*>(smem_raw + S::kActBytes + S::kRedBytes + S::kPtsBytes) + w * (LG * 128) + lane;
  // [NW * RP][P] partial sums of the final reduction.  RS: in the LDS stash -- last read by reverse stage 1, before the
  // barrier that ends it; written again by hidden layer 0 of the next tile, two barriers after the epilogue that reads this.
  f32x4* redf = RS ? reinterpret_cast<f32x4*>(smem_raw + S::kActBytes + S::kRedBytes + S::kPtsBytes) : red;

  // weight images of this wave: forward / transposed image of hidden layer l (two fp16 parts)
  constexpr int FP = 2, BP = 2;
  auto fwd_img = [&](int l) { return reinterpret_cast<const u32x4*>(a.packed + x16_off_layer(H, L, l)) + (TW * w * 2) * 64; };
  auto rev_img = [&](int l) { return reinterpret_cast<const u32x4*>(a.packed + x16_off_bw(H, L, l)) + (TW * w * 2) * 64; };
  // accumulator scale of forward layer l: 2^12 (activations) * 2^s_l (weights)
  auto fwd_scale = [&](int l) { return kActScale * a.packed[x16_base(H, L) + l]; };
  // per-point maxima of the adjoint, exchanged between the waves: [2][P][NW] floats in the (otherwise
  // idle until the final reduction) `red` region
  float* redm = reinterpret_cast<float*>(red);
  float bscale[NB];                           // scale carried by the adjoint that sits in LDS, per point of this lane
  float amax[NB];                             // max |adjoint| over this lane's features, per point
  auto put_amax = [&](int buf) {              // before the barrier that ends the stage
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const float m = __builtin_fmaxf(amax[n], __shfl_xor(amax[n], 32));
      if (h == 0) redm[(buf * P + 32 * n + j) * NW + w] = m;
    }
  };
  // RS: the lane offset of a GEMM stage's operand addresses, opaque per stage.  With the layers expanded every weight
  // address is invariant over the tile loop; left visible, lane + image + K-step offsets are hoisted out of it as
  // 64-bit per-lane pointers, one pair of registers per K-step and image, and spilled.
  auto stage_lane = [&]() __attribute__((always_inline)) {
    int v = lane;
    if constexpr (RS) asm volatile("" : "+v"(v));
    return v;
  };
  u32x4 A[4][TW][3];                     // weight-fragment pipeline, carried across stages
  x3_prefetch_a<kAD, TW, NTO, FP>(A, fwd_img(0), 0, lane);

  // (agent-scope load: in the Newton tail the count was written by this workgroup's own atomics a moment ago)
  const int64_t total = a.count_in ? (int64_t)__hip_atomic_load(a.count_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.n;
  if (total <= a.cnt_lo || total > a.cnt_hi) return;       // the other tile shape serves this list (uniform)
  // ps_guard is always 0 in this library (it served an experimental point-stationary kernel, tools/experiments/siren_ps);
  // the check stays because removing it changes this kernel's machine code
  if (a.ps_guard && H == 256 && siren_ps_takes(total, L, a.packed + x16_base(H, L), a.wh)) return;
  // this launch's share of the list: slots [slot0, count)  (SirenArgs::split)
  const int64_t cut = a.split ? siren_split_point(total) : total;
  const int64_t slot0 = a.split == 2 ? cut : 0;
  const int64_t count = a.split == 1 ? cut : total;
  const int64_t n_tiles = (count - slot0 + P - 1) / P;
  // Tile boundary.  A tile used to end with two chains of dependent loads during which the whole CU
  // idled: the epilogue (list entry -> position -> returning atomic of the survivor list; 4.6 k cycles, one and a
  // half waves busy, the others parked at a closing barrier) and then the next tile's points (list entry -> position,
  // 2.3 k).  Now the next tile's list entries are requested during reverse stage 0 and its positions before the
  // barrier that precedes the epilogue; the epilogue takes the position from LDS (`ptl`) and its list entry from a
  // load issued before that barrier; and the closing barrier is gone -- waves 2..7 start layer 0 of the next tile
  // while waves 0-1 finish the epilogue (no LDS hazard: `red` is next written after three more barriers, `ptl` by
  // wave 0 itself, the activation regions were last read before the barrier that ends reverse stage 0's GEMM).
  __shared__ int s_next_tile, s_first_tile;
  int nidx[NB];
  float npx[NB], npy[NB], npz[NB];
  int nrow[NB];                                          // CODED: the points' rows of the bias table
  auto fetch_idx = [&](int64_t t) {                      // list entries of tile t (-1: beyond the list)
    int j_e = j;
    asm volatile("" : "+v"(j_e));
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int64_t slot = slot0 + t * P + 32 * n + j_e;
      nidx[n] = -1;
      if (t < n_tiles && slot < count) nidx[n] = a.idx_in ? a.idx_in[slot] : (int)slot;
    }
  };
  auto fetch_pts = [&]() {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      npx[n] = npy[n] = npz[n] = 0.f;
      if constexpr (CODED) nrow[n] = 0;
      if (nidx[n] >= 0) {
        const int64_t idx = nidx[n];
        npx[n] = a.pts[idx * 3]; npy[n] = a.pts[idx * 3 + 1]; npz[n] = a.pts[idx * 3 + 2];
        if constexpr (CODED) nrow[n] = a.code_of ? a.code_of[idx] : 0;
      }
    }
  };
  int64_t first_tile = bid;
  if (!FWD && a.tile_ctr != nullptr && a.draw_first) {       // (uniform) the first tile is drawn as well
    if (tid == 0) s_first_tile = atomicAdd(a.tile_ctr, 1);
    __syncthreads();
    first_tile = s_first_tile;
  }
  fetch_idx(first_tile);
  fetch_pts();
  // Which tile comes next.  Static: bid + k nblk -- every CU takes the same number of tiles, and the launch ends with the
  // slowest XCD (under the power cap the eight XCDs of one MI355X ran this kernel 6.8 % apart, measured with per-workgroup clock stamps).
  // Dynamic (a.tile_ctr, reverse kernels): thread 0 draws the next tile from a counter (zero when the launch starts) while
  // stage 0's GEMM runs and hands it to the workgroup through LDS at the barrier that ends that GEMM.  A point's result
  // does not depend on the tile it sits in or on the workgroup that takes the tile.
  const bool dyn = !FWD && a.tile_ctr != nullptr;
  const int draw_base = a.draw_first ? 0 : nblk;
  int64_t next_tile = 0;
  for (int64_t tile = first_tile; tile < n_tiles; tile = next_tile) {
    float px[NB], py[NB], pz[NB];
    int row[NB];
    int j_e = j;
    asm volatile("" : "+v"(j_e));
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      px[n] = npx[n]; py[n] = npy[n]; pz[n] = npz[n];
      if constexpr (CODED) row[n] = nrow[n];
      if constexpr (!FWD) {                // kept for the reverse sweep's layer 0 (visible after the barrier below)
        if constexpr (CODED) {             // (the table row rides in the free 4th component)
          if (w == 0 && h == 0) ptl[32 * n + j_e] = (f32x4){px[n], py[n], pz[n], __int_as_float(row[n])};
        } else {
          if (w == 0 && h == 0) ptl[32 * n + j_e] = (f32x4){px[n], py[n], pz[n], 0.f};
        }
      }
    }
    // ---- layer 0 (3 -> H) on the VALU: this wave's H/NW features of all P points ------------
    for (int sl = 0; sl < SL; ++sl) {
      f32x4 wv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[e] = W0u[sl * 16 + h8 + e];
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        float zz[8], hv[8], sv[8];
        if constexpr (CODED) {
          float bz[8];
          x3_code_bias8<H>(a.code_bias, row[n], SL * w + sl, h, bz);
#pragma unroll
          for (int e = 0; e < 8; ++e) zz[e] = ((wv[e].x * px[n] + wv[e].y * py[n]) + wv[e].z * pz[n]) + bz[e];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) zz[e] = ((wv[e].x * px[n] + wv[e].y * py[n]) + wv[e].z * pz[n]) + wv[e].w;
        }
        x3_sin_wcos8(a.w0, a.w0, zz, hv, sv);
        const int k = sl * NB + n;
        {
          u32x4 p0, p1;
          split8_f16(hv, p0, p1);
          own[(k * kAP + 0) * 64] = p0; own[(k * kAP + 1) * 64] = p1;
        }
        // w cos(w z0) is NOT stashed: z0 = W0 x + b0 is three FMAs to form again in the reverse sweep
        (void)sv;
      }
    }
    __syncthreads();

    f32x16 acc[TW][NB];
    // RS: slots 0 .. LT-2 of the derivative stash, the groups that are not in LDS (static indices only: registers)
    f32x4 rst[RS && LT > 1 ? LT - 1 : 1][RS ? NG : 1][2];
    float fpart[RP][NB];
#pragma unroll
    for (int r = 0; r < RP; ++r)
#pragma unroll
      for (int n = 0; n < NB; ++n) fpart[r][n] = 0.f;
    // ---- hidden layers, forward --------------------------------------------------------------
    auto fwd_layer = [&](auto lc) __attribute__((always_inline)) {
      const int l = lc;                     // (an integral_constant in the on-chip form)
      const int gl = stage_lane();
      const float* lay = a.packed + x3_off_layer(H, L, l);
      const u32x4* img = fwd_img(l);
      const float zscale = fwd_scale(l);             // the accumulators hold zscale * (W h + b)
      const float w_in = a.wh / zscale;              // exact: zscale is a power of two
      if (l + 1 < L || FWD) {
        // the next stage is a forward one again (layer l+1, or layer 0 of the next tile)
        gemm_x3<kAD, TW, NB, NTO, NS, kBias, IL, FP, FP>(img, lay, act + gl, acc, w, 0, A,
                                                         l + 1 < L ? fwd_img(l + 1) : fwd_img(0), 0, gl, zscale);
      } else {
        gemm_x3<kAD, TW, NB, NTO, NS, kBias, IL, FP, BP>(img, lay, act + gl, acc, w, 0, A, rev_img(L - 1), 0, gl,
                                                         zscale);
      }
      __syncthreads();                      // both teams have read this team's K-half
      const bool top = (l == L - 1);
      f32x4* st_l = stash + (int64_t)l * NG * 128;
      const bool lds_slot = (l == 0);        // the first LG groups of slot 0 (the longest-lived one) stay in LDS
      // one 8-value group: sin / w cos, head or stash, split, store as the next layer's B entry
      // scale of the adjoint seed (uniform): |W_head[f] * w cos| <= max|W_head| * w
      const float seed_scale = x3_scale_for(a.packed[x16_base(H, L) + 16] * a.wh * 1.01f);
      if (top) {
#pragma unroll
        for (int n = 0; n < NB; ++n) { amax[n] = 0.f; bscale[n] = seed_scale; }
      }
      auto act_group = [&](int k, int n, int sl, const float (&zz)[8], float& fp) {
        float hv[8], sv[8];
        x3_sin_wcos8(w_in, a.wh, zz, hv, sv);
        if (top) {
          // adjoint seed of the top sine layer = head weight * w cos(w z); head dot product here
          const f32x4 wl0 = *reinterpret_cast<const f32x4*>(WLu + sl * 16 + h8);
          const f32x4 wl1 = *reinterpret_cast<const f32x4*>(WLu + sl * 16 + h8 + 4);
          const float f0 = (wl0.x * hv[0] + wl0.y * hv[1]) + (wl0.z * hv[2] + wl0.w * hv[3]);
          const float f1 = (wl1.x * hv[4] + wl1.y * hv[5]) + (wl1.z * hv[6] + wl1.w * hv[7]);
          fp += f0 + f1;
          // (RS: with the layers expanded the sum has one use, far below, and would be sunk there with the operands of
          // all its groups kept live: 150 registers)
          if constexpr (RS) asm volatile("" : "+v"(fp));
          if constexpr (FWD) return;
#pragma unroll
          for (int e = 0; e < 4; ++e) { hv[e] = wl0[e] * sv[e]; hv[4 + e] = wl1[e] * sv[4 + e]; }
          float m = amax[n];
#pragma unroll
          for (int e = 0; e < 8; e += 2) m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(hv[e]), __builtin_fabsf(hv[e + 1])));
          amax[n] = m;
          u32x4 p0, p1;
          split8_f16(hv, p0, p1, seed_scale);
          own[(k * kAP + 0) * 64] = p0; own[(k * kAP + 1) * 64] = p1;
          return;
        } else {
          if constexpr (!FWD) {
            if (k < LG && lds_slot) {
              lst[(k * 2 + 0) * 64] = (f32x4){sv[0], sv[1], sv[2], sv[3]};
              lst[(k * 2 + 1) * 64] = (f32x4){sv[4], sv[5], sv[6], sv[7]};
            } else if constexpr (RS) {
              if constexpr (LT > 1) {
                rst[l < LT - 1 ? l : 0][k][0] = (f32x4){sv[0], sv[1], sv[2], sv[3]};
                rst[l < LT - 1 ? l : 0][k][1] = (f32x4){sv[4], sv[5], sv[6], sv[7]};
              }
            } else {
              st_l[(k * 2 + 0) * 64 + lane] = (f32x4){sv[0], sv[1], sv[2], sv[3]};
              st_l[(k * 2 + 1) * 64 + lane] = (f32x4){sv[4], sv[5], sv[6], sv[7]};
            }
          }
        }
        u32x4 p0, p1;                           // input of the next forward layer
        split8_f16(hv, p0, p1);
        own[(k * kAP + 0) * 64] = p0; own[(k * kAP + 1) * 64] = p1;
      };
      if constexpr (NG <= 8 || RS) {
        // few enough values per lane to walk the accumulators with static indices (RS: 12 groups, and registers for them)
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int n = 0; n < NB; ++n) {
              float zz[8];
#pragma unroll
              for (int e = 0; e < 8; ++e) zz[e] = acc[t][n][8 * p + e];
              act_group((2 * t + p) * NB + n, n, 2 * t + p, zz, fpart[RS ? t : 0][n]);
              __builtin_amdgcn_sched_barrier(0);     // one group at a time: bounds register pressure
            }
      } else {
        // park the accumulators (f32) in the tail of this wave's own, now dead, LDS region and
        // walk them with a rolled loop; results overwrite the region front to back
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              const int k = (2 * t + p) * NB + n;
              const f32x16& v = acc[t][n];
              park[(k * 2 + 0) * 64] = as_u32x4((f32x4){v[8 * p], v[8 * p + 1], v[8 * p + 2], v[8 * p + 3]});
              park[(k * 2 + 1) * 64] = as_u32x4((f32x4){v[8 * p + 4], v[8 * p + 5], v[8 * p + 6], v[8 * p + 7]});
            }
        for (int sl = 0; sl < SL; ++sl) {
          f32x4 z[NB][2];
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            z[n][0] = as_f32x4(park[((sl * NB + n) * 2 + 0) * 64]);
            z[n][1] = as_f32x4(park[((sl * NB + n) * 2 + 1) * 64]);
          }
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            float zz[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) zz[e] = z[n][e >> 2][e & 3];
            act_group(sl * NB + n, n, sl, zz, fpart[0][n]);
          }
        }
      }
      if constexpr (!FWD) { if (top) put_amax(0); }
      __syncthreads();                      // the next layer's inputs are complete
    };
    if constexpr (RS) {
      static_assert(LT <= 3, "layers are expanded by hand");
      fwd_layer(std::integral_constant<int, 0>());
      if constexpr (LT > 1) fwd_layer(std::integral_constant<int, 1>());
      if constexpr (LT > 2) fwd_layer(std::integral_constant<int, 2>());
    } else {
      for (int l = 0; l < L; ++l) fwd_layer(l);
    }
    // ---- hidden layers, reverse --------------------------------------------------------------
    float gx[RP][NB], gy[RP][NB], gz[RP][NB];
#pragma unroll
    for (int r = 0; r < RP; ++r)
#pragma unroll
      for (int n = 0; n < NB; ++n) gx[r][n] = gy[r][n] = gz[r][n] = 0.f;
    int mbuf = 0;                             // exchange buffer that holds max |a_l| of the adjoint in LDS
    // max_k |a_l[k][p]| of this lane's points (written before the barrier that ended the last stage)
    auto get_amax = [&](float (&Mp)[NB]) {
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        float m = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) m = __builtin_fmaxf(m, redm[(mbuf * P + 32 * n + j) * NW + ww]);
        Mp[n] = m;
      }
    };
    // stages l = L-1 .. 1: a_{l-1} = (W_l^T a_l) * w cos(w z_{l-1}), the derivative from the stash
    auto rev_stage = [&](auto lc) __attribute__((always_inline)) {
      const int l = lc;
      const int gl = stage_lane();
      const u32x4* img = rev_img(l);
      const f32x4* st_l = stash + (int64_t)(l - 1) * NG * 128;      // reverse stage l reads slot l - 1
      f32x4 sv[NG][2];
      auto ld_stash = [&]() {
#pragma unroll
        for (int k = 0; k < NG; ++k) {
          if (k < LG && l == 1) {
            sv[k][0] = lst[(k * 2) * 64]; sv[k][1] = lst[(k * 2 + 1) * 64];
          } else if constexpr (RS) {
            if constexpr (LT > 1) { sv[k][0] = rst[l - 1 < LT - 1 ? l - 1 : 0][k][0]; sv[k][1] = rst[l - 1 < LT - 1 ? l - 1 : 0][k][1]; }
          } else {
            sv[k][0] = st_l[(k * 2) * 64 + lane]; sv[k][1] = st_l[(k * 2 + 1) * 64 + lane];
          }
        }
      };
      float Mp[NB];
      get_amax(Mp);
      gemm_x3<kAD, TW, NB, NTO, NS, kZero, IL, BP, BP>(img, nullptr, act + gl, acc, w, 0, A, rev_img(l - 1), 0, gl);
      ld_stash();                             // w cos(w z) of the layer below
      __syncthreads();
      // split-fp16 reverse: the accumulators hold 2^s_l * bscale[p] * (W_l^T a_l); the scale comes out
      // exactly, the next adjoint gets the scale its bound allows
      float inv[NB], nscale[NB];
      {
        const float iw = 1.0f / a.packed[x16_base(H, L) + l];
        const float grow = a.packed[x16_base(H, L) + 8 + l] * a.wh * 1.01f;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          inv[n] = iw / bscale[n];
          nscale[n] = x3_scale_for(Mp[n] * grow);
          amax[n] = 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            const int k = (2 * t + p) * NB + n;
            float av[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) av[e] = (acc[t][n][8 * p + e] * inv[n]) * sv[k][e >> 2][e & 3];
            float m = amax[n];
#pragma unroll
            for (int e = 0; e < 8; e += 2) m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(av[e]), __builtin_fabsf(av[e + 1])));
            amax[n] = m;
            u32x4 p0, p1;
            split8_f16(av, p0, p1, nscale[n]);
            own[(k * kAP + 0) * 64] = p0; own[(k * kAP + 1) * 64] = p1;
            if constexpr (RS) __builtin_amdgcn_sched_barrier(0);     // one group at a time, as in the forward walk
          }
        }
#pragma unroll
      for (int n = 0; n < NB; ++n) bscale[n] = nscale[n];
      put_amax(mbuf ^ 1);
      mbuf ^= 1;
      __syncthreads();
    };
    if constexpr (RS) {
      if constexpr (LT > 2) rev_stage(std::integral_constant<int, 2>());
      if constexpr (LT > 1) rev_stage(std::integral_constant<int, 1>());
    } else {
      for (int l = FWD ? 0 : L - 1; l >= 1; --l) rev_stage(l);
    }
    // stage 0: d sdf / d x = W_0^T [ (W_1^T a_1) * w0 cos(w0 z_0) ] -- z_0 = W_0 x + b_0 is formed again from the point
    // (three FMAs; the same expression on the same operands as in the forward sweep) instead of being stashed
    if constexpr (!FWD) {
      const int gl = stage_lane();
      int drawn = 0;
      if (dyn && tid == 0) drawn = draw_base + atomicAdd(a.tile_ctr, 1);
      gemm_x3<kAD, TW, NB, NTO, NS, kZero, IL, BP, FP>(rev_img(0), nullptr, act + gl, acc, w, 0, A, fwd_img(0), 0, gl);
      if (dyn && tid == 0) s_next_tile = drawn;
      __syncthreads();
      next_tile = dyn ? (int64_t)s_next_tile : tile + nblk;
      fetch_idx(next_tile);
      float inv[NB];
      {
        const float iw = 1.0f / a.packed[x16_base(H, L)];
#pragma unroll
        for (int n = 0; n < NB; ++n) inv[n] = iw / bscale[n];
      }
      f32x4 q[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) q[n] = ptl[32 * n + j];
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          f32x4 wv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) wv[e] = W0u[(2 * t + p) * 16 + h8 + e];
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            float zz[8], cv[8];
            if constexpr (CODED) {
              float bz[8];
              x3_code_bias8<H>(a.code_bias, __float_as_int(q[n].w), SL * w + 2 * t + p, h, bz);
#pragma unroll
              for (int e = 0; e < 8; ++e) zz[e] = ((wv[e].x * q[n].x + wv[e].y * q[n].y) + wv[e].z * q[n].z) + bz[e];
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) zz[e] = ((wv[e].x * q[n].x + wv[e].y * q[n].y) + wv[e].z * q[n].z) + wv[e].w;
            }
            iso_wcos8(a.w0, a.w0, zz, cv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float av = (acc[t][n][8 * p + e] * inv[n]) * cv[e];
              gx[RS ? t : 0][n] += wv[e].x * av;
              gy[RS ? t : 0][n] += wv[e].y * av;
              gz[RS ? t : 0][n] += wv[e].z * av;
            }
            __builtin_amdgcn_sched_barrier(0);     // one group at a time: bounds register pressure
          }
        }
      // (no barrier here: between the one that ends this stage's GEMM and the one after the
      // reduction nothing reads what the reduction writes)
    } else {
      next_tile = tile + nblk;
      fetch_idx(next_tile);
    }
    // ---- reduce head + gradient over the lane halves and the waves -----------------------------
#pragma unroll
    for (int r = 0; r < RP; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float f = fpart[r][n] + __shfl_xor(fpart[r][n], 32);
      float x = gx[r][n] + __shfl_xor(gx[r][n], 32);
      float y = gy[r][n] + __shfl_xor(gy[r][n], 32);
      float z = gz[r][n] + __shfl_xor(gz[r][n], 32);
      if (h == 0) redf[(RP * w + r) * P + 32 * n + j] = (f32x4){f, x, y, z};
    }
    // (the thread / lane ids are made opaque here: everything derived from them -- LDS addresses,
    // the rank mask of the compaction -- is recomputed per tile instead of being kept live, and
    // spilled, across the whole tile)
    int tid_e = tid, lane_e = lane;
    asm volatile("" : "+v"(tid_e), "+v"(lane_e));
    int eidx = -1;                              // the epilogue's list entry and position, requested
    f32x4 qe = {0.f, 0.f, 0.f, 0.f};            // before the barrier (the position while `ptl` still holds this tile)
    {
      const int64_t slot = slot0 + tile * P + tid_e;
      if (tid_e < P && slot < count) {
        eidx = a.idx_in ? a.idx_in[slot] : (int)slot;
        if constexpr (!FWD) qe = ptl[tid_e];
      }
      fetch_pts();
    }
    __syncthreads();
    // ---- epilogue: thread tid handles point `tid` of the tile ----------------------------------
    bool survive = false;
    int64_t idx = -1;
    {
      const int64_t slot = slot0 + tile * P + tid_e;
      if (tid_e < P && slot < count) {
        f32x4 r = redf[tid_e];
#pragma unroll
        for (int ww = 1; ww < NW * RP; ++ww) {
          const f32x4 q = redf[ww * P + tid_e];
          r.x += q.x; r.y += q.y; r.z += q.z; r.w += q.w;
        }
        const float f = r.x + bL;
        idx = eidx;
        if constexpr (!FWD) survive = iso_step_finish<SirenArgs, true>(a, idx, f, r.y, r.z, r.w, qe.x, qe.y, qe.z);
        else survive = iso_step_finish(a, idx, f, r.y, r.z, r.w);
      }
    }
    if (!a.eval_only && a.do_move) {
      const unsigned long long bal = __ballot(survive);
      if (bal) {
        int base = 0;
        const int leader = __ffsll((long long)bal) - 1;
        if (lane_e == leader) base = atomicAdd(a.count_out, __popcll(bal));
        base = __shfl(base, leader);
        if (survive) {
          const int rank = __popcll(bal & ((1ull << lane_e) - 1ull));
          a.idx_out[base + rank] = (int32_t)idx;
        }
      }
    }
  }
}

template <int H, int NW, int NB, int MINB, bool FWD, bool CODED>
__global__ __launch_bounds__(64 * NW, MINB) void k_siren_step_x3(typename SirenArgsOf<CODED>::type a) {
  x3_step_body<H, NW, NB, FWD, CODED>(a, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.x);
}

// Both tile shapes of a split list (SirenArgs::split) in ONE launch: workgroups [0, big_blocks) serve the slots below
// siren_split_point(count) on NB-tile workgroups, the others the rest on one-tile workgroups (their own stash region
// behind the first group's).  The dispatcher places workgroups in index order, one per CU, so the small tiles start
// on the CUs that finish their large ones first; a launch that finds nothing to do for one of the shapes costs nothing
// (issued separately, the idle one of the two launches took ~4.4 us, 15 times per headline cycle).
template <int H, int NW, int NB, int MINB, bool CODED>
__global__ __launch_bounds__(64 * NW, MINB) void k_siren_step_x3_both(typename SirenArgsOf<CODED>::type a) {
  const bool big = (int)blockIdx.x < a.big_blocks;
  const int small_blocks = (int)gridDim.x - a.big_blocks;
  if (big) {
    typename SirenArgsOf<CODED>::type b = a;
    b.split = 1;
    x3_step_body<H, NW, NB, false, CODED>(b, (int)blockIdx.x, a.big_blocks, (int)blockIdx.x);
  }
  // Drawn tiles (a.tile_ctr): a workgroup of the large shape that finds no large tile left goes on with the small ones
  // (its own stash region, participant small_blocks + blockIdx of small_blocks + big_blocks) -- the large workgroups end
  // within one tile time (68 us) of each other, and the small tiles are what the early ones fill that time with
  // (headline cycle 13.33-13.38 -> 13.22-13.25 ms; with half a round to one and a half rounds of the large tiles' points
  // handed to the small ones on top: 13.26-13.28).
  if (!big || a.tile_ctr != nullptr) {
    if (big) __syncthreads();              // (the last large tile's epilogue reads LDS the other shape lays out differently)
    typename SirenArgsOf<CODED>::type b = a;
    b.split = 2;
    if (a.tile_ctr) b.tile_ctr = a.tile_ctr + 1;
    const bool joint = a.tile_ctr != nullptr;
    b.draw_first = joint ? 1 : 0;          // (a workgroup that joins late must not own a tile nobody else may take)
    const int bid = big ? small_blocks + (int)blockIdx.x : (int)blockIdx.x - a.big_blocks;
    const int nblk = joint ? small_blocks + a.big_blocks : small_blocks;
    if (big) b.stash = a.stash + (int64_t)blockIdx.x * X3Shape<H, NW, NB>::kStashPerWg(a.L);
    else b.stash = a.stash + (int64_t)a.big_blocks * X3Shape<H, NW, NB>::kStashPerWg(a.L);
    x3_step_body<H, NW, 1, false, CODED>(b, bid, nblk, big ? 0 : bid);
  }
}

// The on-chip form (x3_step_body, LT > 0) of the kernel above: four waves, LT hidden layers, no global stash.
// (A kernel of its own, not more parameters of the one above: that keeps its name and its machine code.)
constexpr int kOcNW = 4;
// (k_siren_step_x3_both, without the stash regions; a function of its own taking the argument block by reference: written
// into the kernel, the same text reserves 68 bytes of scratch per lane that no instruction uses)
template <int H, int NB, bool CODED, int LT>
__device__ __forceinline__ void x3_both_oc(const typename SirenArgsOf<CODED>::type& a) {
  const bool big = (int)blockIdx.x < a.big_blocks;
  const int small_blocks = (int)gridDim.x - a.big_blocks;
  if (big) {
    typename SirenArgsOf<CODED>::type b = a;
    b.split = 1;
    x3_step_body<H, kOcNW, NB, false, CODED, LT>(b, (int)blockIdx.x, a.big_blocks, (int)blockIdx.x);
  }
  if (!big || a.tile_ctr != nullptr) {
    if (big) __syncthreads();
    typename SirenArgsOf<CODED>::type b = a;
    b.split = 2;
    if (a.tile_ctr) b.tile_ctr = a.tile_ctr + 1;
    const bool joint = a.tile_ctr != nullptr;
    b.draw_first = joint ? 1 : 0;
    const int bid = big ? small_blocks + (int)blockIdx.x : (int)blockIdx.x - a.big_blocks;
    const int nblk = joint ? small_blocks + a.big_blocks : small_blocks;
    x3_step_body<H, kOcNW, 1, false, CODED, LT>(b, bid, nblk, big ? 0 : bid);
  }
}
template <int H, int NB, int MINB, bool CODED, int LT>
__global__ __launch_bounds__(64 * kOcNW, MINB) void k_siren_step_x3_both_oc(typename SirenArgsOf<CODED>::type a) {
  x3_both_oc<H, NB, CODED, LT>(a);
}

// The Newton tail in ONE launch (levelset_sampling.py:306-341: the reference leaves its loop when nothing is active; a
// launch per iteration issued all T + 1 of them, the late ones for a few hundred points or none).  Iteration it_first
// is taken from the list the previous launch left, dealt out tile by tile (32 points) as always; but a workgroup puts
// the survivors of ITS tiles on a private list and goes on with them alone -- evaluate, move, keep the survivors --
// until none is left or iteration it_last (the evaluation without a move) is done.  A point's result does not depend
// on the tile it sits in, so the results are those of the launch-per-iteration form, bit for bit.  Between two rounds
// one workgroup barrier (the epilogue's atomics and list entries of the slower waves must have landed).
template <int H, int NW, int MINB, bool CODED>
__global__ __launch_bounds__(64 * NW, MINB) void k_siren_tail_x3(typename SirenArgsOf<CODED>::type a) {
  const int b = blockIdx.x, nblk = gridDim.x;
  int32_t* lists = a.tail_lists + (int64_t)b * 2 * a.tail_cap;
  int32_t* cnts = a.tail_counts + b * 2;
  typename SirenArgsOf<CODED>::type r = a;
  r.split = 0; r.small_tiles = 1; r.cnt_lo = -1; r.cnt_hi = INT64_MAX; r.tile_ctr = nullptr;
  // round 0: this workgroup's tiles of the global list
  r.idx_out = lists; r.count_out = cnts;
  r.do_move = a.it_first < a.it_last ? 1 : 0;
  x3_step_body<H, NW, 1, false, CODED>(r, b, nblk, b);
  int cur = 0;
  for (int it = a.it_first + 1; it <= a.it_last; ++it) {
    __syncthreads();
    const int m = __hip_atomic_load(&cnts[cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m == 0) break;                                     // (workgroup-uniform)
    if (threadIdx.x == 0) {
      __hip_atomic_store(&cnts[cur ^ 1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.iter_counts) atomicAdd(&a.iter_counts[it], m);
    }
    __syncthreads();
    r.idx_in = lists + (int64_t)cur * a.tail_cap; r.count_in = cnts + cur;
    r.idx_out = lists + (int64_t)(cur ^ 1) * a.tail_cap; r.count_out = cnts + (cur ^ 1);
    r.do_move = it < a.it_last ? 1 : 0;
    x3_step_body<H, NW, 1, false, CODED>(r, 0, 1, b);
    cur ^= 1;
  }
  // leave the private counters at zero for the next launch on this workspace
  __syncthreads();
  if (threadIdx.x == 0) { cnts[0] = 0; cnts[1] = 0; }
}

template <int H, int NW, int NB, int MINB, bool FWD, bool CODED>
int launch_x3(const typename SirenArgsOf<CODED>::type& a, int64_t n_upper, hipStream_t s) {
  using S = X3Shape<H, NW, NB>;
  static_assert(S::kLds <= 163840, "LDS of a gfx950 CU");
  iso_launch_lds<k_siren_step_x3<H, NW, NB, MINB, FWD, CODED>>(iso_capped_grid(n_upper, S::P, 256 * MINB), 64 * NW, S::kLds, s, a);
  return 0;
}

// LT > 0: the on-chip form of LT hidden layers (NW = kOcNW)
template <int H, int NW, int NB, int MINB, bool CODED, int LT = 0>
int launch_x3_both(typename SirenArgsOf<CODED>::type a, int64_t n_upper, hipStream_t s) {
  constexpr int RP = LT > 0 ? (H / 32) / NW : 1;
  using SB = X3Shape<H, NW, NB, RP>;
  using SS = X3Shape<H, NW, 1, RP>;
  static_assert(LT == 0 || NW == kOcNW, "the on-chip form: four waves");
  constexpr size_t lds = SB::kLds > SS::kLds ? SB::kLds : SS::kLds;
  static_assert(lds <= 163840, "LDS of a gfx950 CU");
  void (*kern)(typename SirenArgsOf<CODED>::type);
  if constexpr (LT > 0) kern = &k_siren_step_x3_both_oc<H, NB, MINB, CODED, LT>;
  else kern = &k_siren_step_x3_both<H, NW, NB, MINB, CODED>;
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_done = true;
  }
  a.big_blocks = iso_capped_grid(n_upper, SB::P, 256 * MINB);
  a.split = 3;                 // (as SirenArgs documents it; the kernel gives each of its two shapes its own 1 / 2)
  const int small_blocks = iso_capped_grid(n_upper, SS::P, 256 * MINB);
  hipLaunchKernelGGL(kern, dim3(a.big_blocks + small_blocks), dim3(64 * NW), lds, s, a);
  return 0;
}

}  // namespace

constexpr int kNW256 = 8;      // waves per workgroup at H = 256
constexpr int kMinB256 = 1;    // workgroups per CU at H = 256
constexpr int kNB256 = 3;      // point tiles of 32 per workgroup at H = 256 (4 would fit LDS with the two-part layout, but needs
                               // 64 + 64 + 32 accumulator / operand registers: 101 spilled VGPRs, 3.63 instead of 3.26 ms)
constexpr int kMinB128 = 1;    // workgroups per CU for H = 128: 2 would fit (78 KiB LDS each) but the 256-VGPR budget then forces
                               // scratch spills, and that build is not repeatable from run to run (tools/siren_repeat_check.py)
bool siren_x3_supported(int H, int L) { return (H == 256 || H == 128) && L >= 1 && L <= 8; }

int64_t siren_x3_stash_floats(int H, int L) {
  if (H == 256) {     // both tile shapes of a split list run in one launch: a region each
    return 256 * kMinB256 * (X3Shape<256, kNW256, kNB256>::kStashPerWg(L) + X3Shape<256, kNW256, 1>::kStashPerWg(L));
  }
  if (H == 128) return 256 * kMinB128 * X3Shape<128, 4, 3>::kStashPerWg(L);
  return 0;
}

void siren_x3_pack(const float* raw, float* packed, int H, int L, hipStream_t s) {
  const int64_t words = x16_base(H, L) - x3_base(H, L);
  hipLaunchKernelGGL(k_siren_pack_x3, dim3(iso_stream_grid(words, 256)), dim3(256), 0, s, raw, packed, H, L);
  if (L > 0) {
    hipLaunchKernelGGL(k_siren_wscale, dim3(L), dim3(256), 0, s, raw, packed, H, L);
    hipLaunchKernelGGL(k_siren_pack_f16, dim3(iso_stream_grid(2 * (int64_t)L * H * H, 256)), dim3(256), 0, s, raw, packed, H, L);
  }
}

int siren_x3_tail_blocks() { return 256 * kMinB256; }

template <bool CODED>
static int launch_tail(const typename SirenArgsOf<CODED>::type& a, hipStream_t s) {
  using SS = X3Shape<256, kNW256, 1>;
  iso_launch_lds<k_siren_tail_x3<256, kNW256, kMinB256, CODED>>(siren_x3_tail_blocks(), 64 * kNW256, SS::kLds, s, a);
  return 0;
}

int siren_x3_launch_tail(const SirenCodedArgs& a, int H, hipStream_t s) {
  if (H != 256) return -1;
  return a.code_bias ? launch_tail<true>(a, s) : launch_tail<false>(a, s);     // (false: the SirenArgs part)
}

// The launch switch of siren_form's codes 2xx .. 5xx (siren.hip: the one place that decides; the table is there).
// The on-chip form (516) exists uncoded only: the coded build is one register short (the allocator parks a lane index in
// an accumulator register, which the code object counts as a spill), and the library ships no new spills.  The H = 256
// gradient kernel of ONE tile shape (k_siren_step_x3<256, ., ., ., false, .>) is not built: every such call is a 416 / 516.
template <bool CODED>
static int launch_form(int form, const typename SirenArgsOf<CODED>::type& a, int64_t n_upper, hipStream_t s) {
  switch (form) {
    case 208: return launch_x3<128, 4, 3, kMinB128, true, CODED>(a, n_upper, s);
    case 216: return launch_x3<256, kNW256, kNB256, kMinB256, true, CODED>(a, n_upper, s);
    case 308: return launch_x3<128, 4, 3, kMinB128, false, CODED>(a, n_upper, s);
    case 416: return launch_x3_both<256, kNW256, kNB256, kMinB256, CODED>(a, n_upper, s);
    case 516:
      if constexpr (!CODED) {
        if (a.L == 2) return launch_x3_both<256, kOcNW, kNB256, kMinB256, false, 2>(a, n_upper, s);
        if (a.L == 3) return launch_x3_both<256, kOcNW, kNB256, kMinB256, false, 3>(a, n_upper, s);
      }
      return -1;
    default: return -1;
  }
}

int siren_x3_launch(int form, const SirenCodedArgs& a, int64_t n_upper, hipStream_t s) {
  return a.code_bias ? launch_form<true>(form, a, n_upper, s) : launch_form<false>(form, a, n_upper, s);   // (false: the SirenArgs part)
}
