// Shared pieces of the fused-MLP kernels (siren_f32.hip, idr_f32.hip): accurate sin/cos and the
// LDS-staged f32 MFMA layer pass.  See siren_f32.hip for the data-layout story.
#pragma once
#include "iso_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- sin/cos ---------------------------------------------------------------
// 3-term Cody-Waite reduction by pi/2 with FMA, cephes-style minimax kernels on
// [-pi/4, pi/4].  Max error ~1 ulp for |x| < 1e4 (tests/test_siren.py checks it
// against float64); larger arguments take the slow libm path.
__device__ __forceinline__ void iso_sincos_core(float x, float& s, float& c) {
  const float two_over_pi = 0.636619772367581343f;
  const float p1 = 1.57079637050628662109375f;        // fl(pi/2)
  const float p2 = -4.37113882867379288655e-8f;       // fl(pi/2 - p1)
  const float p3 = -1.71512451000588187280e-15f;      // fl(pi/2 - p1 - p2)
  float n = rintf(x * two_over_pi);
  float r = __builtin_fmaf(-n, p1, x);
  r = __builtin_fmaf(-n, p2, r);
  r = __builtin_fmaf(-n, p3, r);
  float r2 = r * r;
  float ps = __builtin_fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = __builtin_fmaf(ps, r2, -1.6666654611e-1f);
  float sr = __builtin_fmaf(ps * r2, r, r);
  float pc = __builtin_fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = __builtin_fmaf(pc, r2, 4.166664568298827e-2f);
  float cr = __builtin_fmaf(pc, r2 * r2, __builtin_fmaf(-0.5f, r2, 1.0f));
  int q = (int)n;
  float ss = (q & 1) ? cr : sr;
  float cc = (q & 1) ? sr : cr;
  s = (q & 2) ? -ss : ss;
  c = ((q + 1) & 2) ? -cc : cc;
}

__device__ __forceinline__ void iso_sincos(float x, float& s, float& c) {
  if (!(fabsf(x) < 1.0e4f)) {
    sincosf(x, &s, &c);
    return;
  }
  iso_sincos_core(x, s, c);
}

typedef float iso_f32x2 __attribute__((ext_vector_type(2)));

// Four pairs at once, STEP-major: a packed f32 op whose result feeds the next instruction costs a
// wait state on gfx950 (the compiler pads the chain of one pair with s_nop: 40 per 8 values, 20 %
// of the issue slots of the activation stage), so every step is written across the four
// independent pairs, with a scheduling barrier behind each step.
#define ISO_X4(expr) _Pragma("unroll") for (int p = 0; p < 4; ++p) { expr; } __builtin_amdgcn_sched_barrier(0)

// Eight arguments at once: the hardware sin / cos path for all, then ONE wave-uniform branch for the
// (practically never taken) large-argument fix-up.  s = sin(w_in*z), c = w*cos(w_in*z)
// (w_in = w except where z carries a power-of-two scale that w_in takes out again).
__device__ __forceinline__ void iso_sin_wcos8(float w_in, float w, const float (&z)[8], float (&s)[8], float (&c)[8]) {
  const iso_f32x2 w2 = {w, w}, wi2 = {w_in, w_in};
  iso_f32x2 x[4], s2[4], c2[4];
  ISO_X4(x[p] = ((iso_f32x2){z[2 * p], z[2 * p + 1]}) * wi2);
  // v_sin_f32 / v_cos_f32 take revolutions and are good to 1.25e-7 absolute on [-1/2, 1/2]
  // (tools/probes/hw_sincos_accuracy.hip: mean error 2.8e-8, a correctly rounded result has 1.5e-8), so
  // only the reduction is done in software: f = x/(2 pi) - rint(x/(2 pi)) with a two-term 1/(2 pi)
  // (the product x * hi is exact inside the fma).  7 issue slots per value instead of 15.5 for the packed
  // polynomial form of iso_sincos_core.
  {
    const iso_f32x2 hi = {0.159154936671257019043f, 0.159154936671257019043f};
    const iso_f32x2 lo = {6.4206383167e-9f, 6.4206383167e-9f};
    iso_f32x2 t[4], n[4], f[4];
    ISO_X4(t[p] = x[p] * hi);
    ISO_X4(n[p] = ((iso_f32x2){rintf(t[p].x), rintf(t[p].y)}));
    ISO_X4(f[p] = __builtin_elementwise_fma(x[p], hi, -n[p]));
    ISO_X4(f[p] = __builtin_elementwise_fma(x[p], lo, f[p]));
    ISO_X4(s2[p] = ((iso_f32x2){__builtin_amdgcn_sinf(f[p].x), __builtin_amdgcn_sinf(f[p].y)}));
    ISO_X4(c2[p] = ((iso_f32x2){__builtin_amdgcn_cosf(f[p].x), __builtin_amdgcn_cosf(f[p].y)}));
  }
  ISO_X4(c2[p] = c2[p] * w2);
  float amax = 0.f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    s[2 * p] = s2[p].x; s[2 * p + 1] = s2[p].y;
    c[2 * p] = c2[p].x; c[2 * p + 1] = c2[p].y;
    amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(x[p].x), __builtin_fabsf(x[p].y)));   // one v_max3
  }
  const bool big = !(amax < 1.0e4f);                 // also true for NaN arguments
  if (__builtin_expect(__any(big), 0)) {
    // |x| >= 1e4 (never seen with trained SIRENs): libm's Payne-Hanek path, one rolled copy
    float xs[8], ss[8], cs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { xs[e] = w_in * z[e]; ss[e] = s[e]; cs[e] = c[e]; }
#pragma unroll 1
    for (int e = 0; e < 8; ++e) {
      float x = xs[0], s0, c0;
      sincosf(x, &s0, &c0);
      const bool fix = !(fabsf(x) < 1.0e4f);
      const float sn = fix ? s0 : ss[0], cn = fix ? w * c0 : cs[0];
      // rotate so that the loop body only ever touches element 0 (static register indices)
#pragma unroll
      for (int i = 0; i < 7; ++i) { xs[i] = xs[i + 1]; ss[i] = ss[i + 1]; cs[i] = cs[i + 1]; }
      xs[7] = x; ss[7] = sn; cs[7] = cn;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] = ss[e]; c[e] = cs[e]; }
  }
}

// c = w*cos(w_in*z) alone, bit for bit the c of iso_sin_wcos8 (same reduction, same instructions): the reverse sweep
// of the SIREN step recomputes layer 0's derivative from the point instead of reading it back from a stash.
__device__ __forceinline__ void iso_wcos8(float w_in, float w, const float (&z)[8], float (&c)[8]) {
  const iso_f32x2 w2 = {w, w}, wi2 = {w_in, w_in};
  iso_f32x2 x[4], c2[4];
  ISO_X4(x[p] = ((iso_f32x2){z[2 * p], z[2 * p + 1]}) * wi2);
  {
    const iso_f32x2 hi = {0.159154936671257019043f, 0.159154936671257019043f};
    const iso_f32x2 lo = {6.4206383167e-9f, 6.4206383167e-9f};
    iso_f32x2 t[4], n[4], f[4];
    ISO_X4(t[p] = x[p] * hi);
    ISO_X4(n[p] = ((iso_f32x2){rintf(t[p].x), rintf(t[p].y)}));
    ISO_X4(f[p] = __builtin_elementwise_fma(x[p], hi, -n[p]));
    ISO_X4(f[p] = __builtin_elementwise_fma(x[p], lo, f[p]));
    ISO_X4(c2[p] = ((iso_f32x2){__builtin_amdgcn_cosf(f[p].x), __builtin_amdgcn_cosf(f[p].y)}));
  }
  ISO_X4(c2[p] = c2[p] * w2);
  float amax = 0.f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    c[2 * p] = c2[p].x; c[2 * p + 1] = c2[p].y;
    amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(x[p].x), __builtin_fabsf(x[p].y)));
  }
  if (__builtin_expect(__any(!(amax < 1.0e4f)), 0)) {
    float s[8];
    iso_sin_wcos8(w_in, w, z, s, c);          // the large-argument path: rare, take the full routine
  }
}

template <int V> struct IsoInt { static constexpr int value = V; };

template <int NT, bool HAS_BIAS>
__device__ __forceinline__ void gemm_pass(const float* __restrict__ img,
                                          const float* __restrict__ bias,
                                          const float* __restrict__ hL,
                                          float* __restrict__ wbuf, f32x4 (&acc)[NT],
                                          int lane, int g) {
  // One pass = NT q-chunks of 16 input features (a square H x H layer: the chunk count used to be a parameter that no
  // caller passed); each q-chunk is staged in two halves of TC = NT/2 tiles so
  // that the LDS stage is 2 x (NT/2) KiB and two workgroups fit on a CU.  All A
  // fragments of a half are requested up front (TC ds_read_b128 in flight) and the MFMAs
  // consume them as they land.  (Without the LDS stage -- every wave streaming its own fragments from L2, no barrier --
  // the pass measured 84 instead of 98 TFLOP/s on the bench workload.)
  //
  // Order of the sums.  An output is NOT one fmaf chain over all H inputs: the even q-chunks go to one accumulator
  // (which starts at the bias), the odd ones to a second, and the two are added at the end.  One chain of H roundings
  // put the mean gradient error of an 8-layer network at 1.6 .. 1.7 x that of torch's float32 path against float64
  // (tests/test_siren_forms_gpu.py; restated in numpy the chain alone reproduces the figure, the sine does not matter);
  // two chains of H / 2 measure 1.3 x (the split-fp16 kernels, whose MFMA sums 16 exact products per rounding: 1.25 x).
  // To keep the registers of one accumulator per tile, the pass takes the two halves of the output tiles one after the
  // other -- all q-chunks of tiles 0 .. TC-1, then all of tiles TC .. NT-1: the same half-chunks through the same two LDS
  // buffers with the same barriers, in another order (NT = 16: 228 VGPRs instead of 204, still two workgroups per CU).
  constexpr int TC = NT / 2;              // tiles per staged half
  constexpr int CH = TC * 256;            // floats per half-chunk
  constexpr int NV = CH / 4;              // float4 per half-chunk
  constexpr int PER = (NV + 255) / 256;   // float4 per thread per half-chunk
  constexpr int NC = 2 * NT;              // half-chunks of the pass
  static_assert(NT % 2 == 0, "NT must be even");
  const int tid = threadIdx.x;
  constexpr bool FULL = (NV % 256) == 0;  // every thread moves PER float4 (no tail guard)
  // position i of the schedule -> half-chunk of the image (laid out [q][half]): i < NT is (q = i, half 0), then half 1
  auto chunk_of = [](int i) { return i < NT ? 2 * i : 2 * (i - NT) + 1; };
  // Two register sets: the global loads of half-chunk i+2 are issued while half-chunk i is
  // multiplied and half-chunk i+1 (loaded one stage earlier) is written to the other LDS buffer,
  // so a load has two MFMA stages (~2k cycles) to land before it is needed.
  f32x4 sx[PER], sy[PER];
  auto gload = [&](f32x4 (&r)[PER], int i) {
    const f32x4* src = reinterpret_cast<const f32x4*>(img + (int64_t)chunk_of(i) * CH);
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (FULL || tid + 256 * k < NV) r[k] = src[tid + 256 * k];
  };
  auto lwrite = [&](const f32x4 (&r)[PER], int buf) {
    f32x4* dst = reinterpret_cast<f32x4*>(wbuf + buf * CH);
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (FULL || tid + 256 * k < NV) dst[tid + 256 * k] = r[k];
  };
  auto stage = [&](int buf, const f32x4& b4, f32x4 (&part)[TC]) {
    const f32x4* wa = reinterpret_cast<const f32x4*>(wbuf + buf * CH);
    f32x4 a4[TC];
#pragma unroll
    for (int t = 0; t < TC; ++t) a4[t] = wa[t * 64 + lane];
    // keep the TC reads ahead of the MFMA block: the scheduler otherwise sinks each read
    // next to its consumer (2 in flight, full LDS latency exposed every 8 MFMAs)
    __builtin_amdgcn_sched_barrier(0);
    // k-major: consecutive MFMAs hit different accumulators (32 cycles issue, 40 dependent latency)
#pragma unroll
    for (int t = 0; t < TC; ++t) part[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[t].x, b4.x, part[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TC; ++t) part[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[t].y, b4.y, part[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TC; ++t) part[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[t].z, b4.z, part[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TC; ++t) part[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[t].w, b4.w, part[t], 0, 0, 0);
    // ... and the LDS write + barrier of the next chunk BEHIND it (hoisted, they make the wave
    // drain all of its reads with only a few MFMAs in flight)
    __builtin_amdgcn_sched_barrier(0);
  };
  // the output tiles half * TC .. + TC - 1: the schedule's positions half * NT .. + NT - 1, two per trip
  auto run_half = [&](auto half_c) {
    constexpr int half = decltype(half_c)::value;
    f32x4 even[TC], odd[TC];
#pragma unroll
    for (int t = 0; t < TC; ++t) {
      if constexpr (HAS_BIAS) {
        even[t] = *reinterpret_cast<const f32x4*>(bias + 16 * (half * TC + t) + 4 * g);
      } else {
        even[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      odd[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    for (int q = 0; q < NT; q += 2) {
      const int i = half * NT + q;
      // ---- q even: half-chunk i in buffer 0; sx holds half-chunk i+1
      const f32x4 b4e = reinterpret_cast<const f32x4*>(hL)[q * 64 + lane];
      if (i + 2 < NC) gload(sy, i + 2);
      stage(0, b4e, even);
      lwrite(sx, 1);
      __syncthreads();
      // ---- q odd: half-chunk i+1 in buffer 1; sy holds half-chunk i+2
      const f32x4 b4o = reinterpret_cast<const f32x4*>(hL)[(q + 1) * 64 + lane];
      if (i + 3 < NC) gload(sx, i + 3);
      stage(1, b4o, odd);
      if (i + 2 < NC) lwrite(sy, 0);
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[half * TC + t] = even[t] + odd[t];
  };
  gload(sx, 0);
  lwrite(sx, 0);
  gload(sx, 1);
  __syncthreads();
  // the wave in its MFMA phase outranks a co-resident wave that is in a VALU (sin/cos) phase:
  // +2 % measured (98.2 -> 100.2 TFLOP/s); the two workgroups of a CU stay better interleaved
  __builtin_amdgcn_s_setprio(1);
  run_half(IsoInt<0>());
  run_half(IsoInt<1>());
  __builtin_amdgcn_s_setprio(0);
}



// Register-pipelined form of gemm_pass (used by idr_f32.hip: one workgroup per CU, so nothing else hides
// an LDS round trip).  Same staging protocol -- half q-chunks through two LDS buffers, one barrier
// per half -- but the A fragments of half-chunk c+1 are read from LDS into a second register set
// WHILE half-chunk c is multiplied (they were published by the previous barrier), the global loads
// of chunk c+3 and the LDS store of chunk c+2 ride behind the same MFMAs (sched_group_barrier), and
// the four k-steps of a tile are issued k-major so that consecutive MFMAs never hit the same
// accumulator (v_mfma_f32_16x16x4_f32: 32 cycles issue but 40 cycles dependent latency).
template <int NT, bool HAS_BIAS>
__device__ __forceinline__ void gemm_pass_pipe(const float* __restrict__ img,
                                               const float* __restrict__ bias,
                                               const float* __restrict__ hL,
                                               float* __restrict__ wbuf, f32x4 (&acc)[NT],
                                               int lane, int g, int nq = NT) {
  constexpr int TC = NT / 2;              // tiles per staged half
  constexpr int CH = TC * 256;            // floats per half-chunk
  constexpr int NV = CH / 4;              // float4 per half-chunk
  constexpr int PER = (NV + 255) / 256;   // float4 per thread per half-chunk
  constexpr bool FULL = (NV % 256) == 0;
  static_assert(NT % 2 == 0, "NT must be even");
  const int tid = threadIdx.x;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if constexpr (HAS_BIAS) {
      acc[t] = *reinterpret_cast<const f32x4*>(bias + 16 * t + 4 * g);
    } else {
      acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  f32x4 F[2][TC], G[2][PER];
  auto gload = [&](f32x4 (&r)[PER], int c) {
    const f32x4* src = reinterpret_cast<const f32x4*>(img + (int64_t)c * CH);
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (FULL || tid + 256 * k < NV) r[k] = src[tid + 256 * k];
  };
  auto lwrite = [&](const f32x4 (&r)[PER], int buf) {
    f32x4* dst = reinterpret_cast<f32x4*>(wbuf + buf * CH);
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (FULL || tid + 256 * k < NV) dst[tid + 256 * k] = r[k];
  };
  auto fread = [&](f32x4 (&f)[TC], int buf) {
    const f32x4* wa = reinterpret_cast<const f32x4*>(wbuf + buf * CH);
#pragma unroll
    for (int t = 0; t < TC; ++t) f[t] = wa[t * 64 + lane];
  };
  auto mma = [&](const f32x4 (&f)[TC], int half, const f32x4& b4) {
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[half * TC + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].x, b4.x, acc[half * TC + t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[half * TC + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].y, b4.y, acc[half * TC + t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[half * TC + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].z, b4.z, acc[half * TC + t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[half * TC + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].w, b4.w, acc[half * TC + t], 0, 0, 0);
  };
  auto pattern = [&]() {
    // [2 MFMA, 1 LDS read] x TC, [MFMA, global load] x PER, [MFMA, LDS store] x PER, rest MFMAs
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
  };
  const int nc = 2 * nq;
  // prologue: chunk 0 -> buffer 0 -> F[0]; chunk 1 -> buffer 1; chunk 2 in flight in G[0]
  gload(G[0], 0);
  lwrite(G[0], 0);
  if (nc > 1) gload(G[1], 1);
  __syncthreads();
  fread(F[0], 0);
  if (nc > 1) lwrite(G[1], 1);
  if (nc > 2) gload(G[0], 2);
  f32x4 b4 = reinterpret_cast<const f32x4*>(hL)[lane];
  __syncthreads();
  for (int q = 0; q < nq; ++q) {
    const int c = 2 * q;
    // ---- half 0: multiply chunk c (F[0]); fetch chunk c+1 fragments, request chunk c+3, store chunk c+2
    if (c + 1 < nc) fread(F[1], 1);
    if (c + 3 < nc) gload(G[1], c + 3);
    mma(F[0], 0, b4);
    if (c + 2 < nc) lwrite(G[0], 0);
    pattern();
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    // ---- half 1: multiply chunk c+1 (F[1]); fetch chunk c+2 fragments, request chunk c+4, store chunk c+3
    f32x4 b4n = b4;
    if (q + 1 < nq) b4n = reinterpret_cast<const f32x4*>(hL)[(q + 1) * 64 + lane];
    if (c + 2 < nc) fread(F[0], 0);
    if (c + 4 < nc) gload(G[0], c + 4);
    mma(F[1], 1, b4);
    if (c + 3 < nc) lwrite(G[1], 1);
    pattern();
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    b4 = b4n;
  }
}
