// Fused SIREN SDF + gradient evaluation and Newton step on the f32 matrix cores
// (v_mfma_f32_16x16x4_f32), gfx950: the packing of the f32 weight images and k_siren_step (siren_form's codes 1xx;
// siren.hip decides, drives the iterations and holds the C ABI).
//
// Reference semantics: Siren.forward (DSS/models/common.py:140-165, SineLayer
// :86-87) evaluated with autograd.grad inside
// UniformProjection._compute_sdf_and_grad (levelset_sampling.py:142-170) and
// iterated by _project_points (:313-342).
//
// Work decomposition
//   * one wave = 16 points.  A hidden layer H->H is the GEMM
//       Z[H x 16pts] = W[H x H] . Hin[H x 16pts]
//     tiled as NT = H/16 output tiles of 16 rows; each 16x16x4 MFMA contracts 4
//     input features.  With the D-layout of that instruction (lane = 16g + j
//     holds rows 4g..4g+3 of column j) the register i of output tile t in lane
//     (g,j) is feature 16t+4g+i of point j -- which is exactly what the NEXT
//     layer's B operand wants for k-step (q=t, i) (B[k=g][j]).  So activations
//     never change lanes between layers: they are kept per wave in LDS as
//     hL[q][lane][0..3] (16 B per lane, lane-linear, conflict-free) and the B
//     operands of four consecutive k-steps are one ds_read_b128.
//   * the A operand (weights) is pre-arranged by iso_siren_pack_weights into a
//     lane-linear image FW[q][t][lane][0..3] (and its transpose BW for the
//     reverse sweep), so one q-chunk of all NT tiles is a contiguous NT KiB
//     block.  The 4 waves of a workgroup share it through a double-buffered
//     LDS stage (global -> registers -> LDS, one barrier per chunk).
//   * reverse-mode gradient: the forward sweep stashes s = w*cos(w*z) of every
//     sine layer in a per-wave scratch (L2 / Infinity-Cache resident, 1 KiB
//     coalesced rows); the reverse sweep multiplies the running adjoint by it
//     and runs the same GEMM loop on the transposed image.
//   * Newton: one launch = one evaluation (+ move) over the list of still
//     active points; survivors are appended to the next list with a wave
//     aggregated atomic, so converged points cost nothing in later launches
//     (the reference's boolean-mask compaction, without host syncs).
//
// Arithmetic: 2*H*H MAC per hidden layer and point (forward + reverse) on the
// matrix cores; layer 0 (3->H), the head (H->1) and sin/cos on the VALU.
#include "siren_common.h"
#include "iso_newton.h"
#include "mlp_common.h"

namespace {

// raw layout: W0[H*3] b0[H] {Wi[H*H] bi[H]}*L WL[H] bL[1]
__global__ void k_siren_pack(const float* __restrict__ raw, float* __restrict__ packed,
                             int H, int L) {
  const int64_t total = off_hidden(H, L);
  const int64_t HH = (int64_t)H * H;
  const int NT = H / 16;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (o < off_wl(H)) {
      // W0img[g][e][c]: c<3 -> W0[f][c], c==3 -> b0[f];  f = 16*(e>>2)+4g+(e&3)
      int64_t k = o;
      int c = (int)(k & 3);
      int e = (int)((k >> 2) % (H / 4));
      int g = (int)((k >> 2) / (H / 4));
      int f = 16 * (e >> 2) + 4 * g + (e & 3);
      v = (c < 3) ? raw[f * 3 + c] : raw[(int64_t)H * 3 + f];
    } else if (o < off_bl(H)) {
      int64_t k = o - off_wl(H);
      int e = (int)(k % (H / 4));
      int g = (int)(k / (H / 4));
      int f = 16 * (e >> 2) + 4 * g + (e & 3);
      const int64_t raw_wl = (int64_t)H * 4 + (int64_t)L * (HH + H);
      v = raw[raw_wl + f];
    } else if (o < off_hidden(H, 0)) {
      const int64_t raw_wl = (int64_t)H * 4 + (int64_t)L * (HH + H);
      v = (o == off_bl(H)) ? raw[raw_wl + H] : 0.f;
    } else {
      int64_t k = o - off_hidden(H, 0);
      const int64_t per = H + 2 * HH;
      int l = (int)(k / per);
      int64_t w = k % per;
      const float* Wl = raw + (int64_t)H * 4 + (int64_t)l * (HH + H);
      const float* bl = Wl + HH;
      if (w < H) {
        v = bl[w];
      } else {
        w -= H;
        bool bwd = w >= HH;
        if (bwd) w -= HH;
        // image index: [q][t][lane][i]
        int i = (int)(w & 3);
        int lane = (int)((w >> 2) & 63);
        int t = (int)((w >> 8) % NT);
        int q = (int)((w >> 8) / NT);
        int a = 16 * t + (lane & 15);            // tile row
        int b = 16 * q + 4 * (lane >> 4) + i;    // contraction index
        v = bwd ? Wl[(int64_t)b * H + a]         // BW: out=b (contracted), in=a
                : Wl[(int64_t)a * H + b];        // FW: out=a, in=b (contracted)
      }
    }
    packed[o] = v;
  }
}

// ---- the step kernel -------------------------------------------------------
#define ISO_GEMM_FWD(img, bias) gemm_pass<NT, true>(img, bias, hL, wbuf, acc, lane, g)
#define ISO_GEMM_BWD(img) gemm_pass<NT, false>(img, nullptr, hL, wbuf, acc, lane, g)

// CODED: layer 0's bias is row code_of[idx] of the per-code table a.code_bias (SirenCodedArgs) instead of the image's
// bias slot; the expression is the same, so a coded evaluation equals the uncoded one of the network whose b0 is that row
template <int NT, bool CODED>
__global__ __launch_bounds__(256, 2) void k_siren_step(typename SirenArgsOf<CODED>::type a) {
  constexpr int H = NT * 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, j = lane & 15;
  float* hL = smem + wave * (NT * 256);
  float* wbuf = smem + 4 * NT * 256;   // 2 x (NT/2) KiB stage
  const float* W0img = a.packed + off_w0(H);
  const float* WLimg = a.packed + off_wl(H);
  const float bL = a.packed[off_bl(H)];
  float* stash = a.stash + ((int64_t)blockIdx.x * 4 + wave) * (int64_t)(a.L + 1) * NT * 256;

  const int64_t count = a.count_in ? (int64_t)(*a.count_in) : a.n;
  const int64_t n_tiles = (count + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t slot = tile * 64 + wave * 16 + j;
    const bool valid = slot < count;
    int64_t idx = -1;
    float px = 0.f, py = 0.f, pz = 0.f;
    int row = 0;
    if (valid) {
      idx = a.idx_in ? (int64_t)a.idx_in[slot] : slot;
      px = a.pts[idx * 3]; py = a.pts[idx * 3 + 1]; pz = a.pts[idx * 3 + 2];
      if constexpr (CODED) row = a.code_of ? a.code_of[idx] : 0;
    }
    // this lane's 4 features 16 e4 + 4g .. +3 of the code's bias row: one 16-B load per e4
    const f32x4* cb = nullptr;
    if constexpr (CODED) cb = reinterpret_cast<const f32x4*>(a.code_bias + (int64_t)row * H) + g;
    (void)cb;
    // ---- layer 0 (3 -> H) on the VALU -------------------------------------
    // The TOP sine layer needs no stash: its adjoint seed is the head weight, so
    // gs = WL * w cos(w z) is formed on the spot (and the head dot product with it).
    float f = 0.f;
    const bool top0 = (a.L == 0);
    for (int e4 = 0; e4 < NT; ++e4) {
      f32x4 h4, s4;
      f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
      if constexpr (CODED) b4 = cb[4 * e4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 w = reinterpret_cast<const f32x4*>(W0img)[g * (H / 4) + e4 * 4 + i];
        float z;
        if constexpr (CODED) z = ((w.x * px + w.y * py) + w.z * pz) + b4[i];
        else z = ((w.x * px + w.y * py) + w.z * pz) + w.w;
        float s, c;
        iso_sincos(a.w0 * z, s, c);
        h4[i] = s;
        s4[i] = a.w0 * c;
      }
      if (top0) {
        const f32x4 w4 = reinterpret_cast<const f32x4*>(WLimg)[g * NT + e4];
        f += (w4.x * h4.x + w4.y * h4.y) + (w4.z * h4.z + w4.w * h4.w);
        h4 = (f32x4){w4.x * s4.x, w4.y * s4.y, w4.z * s4.z, w4.w * s4.w};
      }
      reinterpret_cast<f32x4*>(hL)[e4 * 64 + lane] = h4;
      if (!top0) reinterpret_cast<f32x4*>(stash)[e4 * 64 + lane] = s4;
    }
    // ---- hidden layers, forward -------------------------------------------
    f32x4 acc[NT];
    for (int l = 0; l < a.L; ++l) {
      const float* base = a.packed + off_hidden(H, l);
      ISO_GEMM_FWD(base + H, base);
      float* st_l = stash + (int64_t)(l + 1) * NT * 256;
      const bool top = (l == a.L - 1);
      // pre-activations go back to this wave's LDS slab (static register
      // indices), then a rolled loop applies sin / stashes w*cos
#pragma unroll
      for (int t = 0; t < NT; ++t) reinterpret_cast<f32x4*>(hL)[t * 64 + lane] = acc[t];
      for (int e4 = 0; e4 < NT; ++e4) {
        const f32x4 z4 = reinterpret_cast<const f32x4*>(hL)[e4 * 64 + lane];
        f32x4 h4, s4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float s, c;
          iso_sincos(a.wh * z4[i], s, c);
          h4[i] = s;
          s4[i] = a.wh * c;
        }
        if (top) {
          const f32x4 w4 = reinterpret_cast<const f32x4*>(WLimg)[g * NT + e4];
          f += (w4.x * h4.x + w4.y * h4.y) + (w4.z * h4.z + w4.w * h4.w);
          h4 = (f32x4){w4.x * s4.x, w4.y * s4.y, w4.z * s4.z, w4.w * s4.w};
          reinterpret_cast<f32x4*>(hL)[e4 * 64 + lane] = h4;
        } else {
          reinterpret_cast<f32x4*>(hL)[e4 * 64 + lane] = h4;
          reinterpret_cast<f32x4*>(st_l)[e4 * 64 + lane] = s4;
        }
      }
    }
    // ---- head: finish the dot product across the 4 lane groups ---------------
    f += __shfl_xor(f, 16);
    f += __shfl_xor(f, 32);
    f += bL;
    // ---- hidden layers, reverse -------------------------------------------
    for (int l = a.L - 1; l >= 0; --l) {
      const float* base = a.packed + off_hidden(H, l);
      ISO_GEMM_BWD(base + H + (int64_t)H * H);
      const float* st_l = stash + (int64_t)l * NT * 256;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 s4 = reinterpret_cast<const f32x4*>(st_l)[t * 64 + lane];
        f32x4 gs = {acc[t].x * s4.x, acc[t].y * s4.y, acc[t].z * s4.z, acc[t].w * s4.w};
        reinterpret_cast<f32x4*>(hL)[t * 64 + lane] = gs;
      }
    }
    // ---- layer 0 reverse: grad = W0^T (adjoint . s0) ------------------------
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int e4 = 0; e4 < NT; ++e4) {
      const f32x4 a4 = reinterpret_cast<const f32x4*>(hL)[e4 * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 w = reinterpret_cast<const f32x4*>(W0img)[g * (H / 4) + e4 * 4 + i];
        gx += w.x * a4[i];
        gy += w.y * a4[i];
        gz += w.z * a4[i];
      }
    }
    gx += __shfl_xor(gx, 16); gx += __shfl_xor(gx, 32);
    gy += __shfl_xor(gy, 16); gy += __shfl_xor(gy, 32);
    gz += __shfl_xor(gz, 16); gz += __shfl_xor(gz, 32);

    // ---- epilogue ----------------------------------------------------------
    bool survive = false;
    if (valid && g == 0) survive = iso_step_finish(a, idx, f, gx, gy, gz);
    if (!a.eval_only && a.do_move) {
      const unsigned long long bal = __ballot(survive);
      if (bal) {
        int base = 0;
        const int leader = __ffsll((long long)bal) - 1;
        if (lane == leader) base = atomicAdd(a.count_out, __popcll(bal));
        base = __shfl(base, leader);
        if (survive) {
          const int rank = __popcll(bal & ((1ull << lane) - 1ull));
          a.idx_out[base + rank] = (int32_t)idx;
        }
      }
    }
    __syncthreads();
  }
}

constexpr int kSirenBlocks = 512;  // persistent: two workgroups per CU (80 KiB LDS each)

template <int NT, bool CODED>
int launch_step(const typename SirenArgsOf<CODED>::type& a, int blocks, hipStream_t s) {
  iso_launch_lds<k_siren_step<NT, CODED>>(blocks, 256, (size_t)(5 * NT * 256) * sizeof(float), s, a);
  return 0;
}

template <bool CODED>
int dispatch_step(const typename SirenArgsOf<CODED>::type& a, int H, int blocks, hipStream_t s) {
  switch (H / 16) {
    case 4: return launch_step<4, CODED>(a, blocks, s);
    case 8: return launch_step<8, CODED>(a, blocks, s);
    case 16: return launch_step<16, CODED>(a, blocks, s);
    default: return -1;
  }
}
}  // namespace

void siren_f32_pack(const float* raw, float* packed, int H, int L, hipStream_t s) {
  hipLaunchKernelGGL(k_siren_pack, dim3(iso_stream_grid(off_hidden(H, L), 256)), dim3(256), 0, s, raw, packed, H, L);
}

int64_t siren_f32_stash_floats(int H, int L) { return (int64_t)kSirenBlocks * 4 * (L + 1) * H * 16; }

int siren_f32_launch(const SirenCodedArgs& a, int H, int64_t n, hipStream_t s) {
  const int64_t tiles = (n + 63) / 64;
  const int blocks = (int)(tiles < kSirenBlocks ? tiles : kSirenBlocks);
  return a.code_bias ? dispatch_step<true>(a, H, blocks, s) : dispatch_step<false>(a, H, blocks, s);
}
