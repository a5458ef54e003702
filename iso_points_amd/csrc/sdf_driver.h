// Host side shared by the fused SDF families (siren.hip, idr.hip): what a projection, trace or evaluation call asks for,
// the checks both make of it, and the ONE launch schedule -- launch `it` evaluates the list launch it-1 left (device-side
// counts, no host read) on a pair of ping-pong lists; the last one does not move.
#pragma once
#include "iso_common.h"

constexpr int kSdfMaxIters = 60;     // counts[] has 64 slots: counts[it] = size of the list launch `it` consumes

struct SdfCall {
  const char* who;                   // the ABI entry, for messages
  const float* pts_in;               // start points / ray origins
  float* pts_out; float* normals_out; uint8_t* mask_out; float* sdf_out; float* grad_out;
  int64_t n;
  int max_iters;
  float tol;
  bool eval_only;                    // one evaluation into sdf_out (+ grad_out), nothing moves
  const float* dirs = nullptr;       // sphere tracing: unit ray directions; null: Newton projection / evaluation
  float alpha = 1.f, bound = 0.f;
  bool trace() const { return dirs != nullptr; }
  // forward sweep only where the family has such a kernel: tracing, and an evaluation without grad_out
  bool value_only() const { return trace() || (eval_only && !grad_out); }
};

// The checks that follow a family's shape check.  1: nothing to do (n == 0), the caller returns ISO_OK.
inline int sdf_call_check(const SdfCall& c, bool ptrs_ok) {
  ISO_REQUIRE(c.n >= 0 && c.max_iters >= 0 && c.max_iters <= kSdfMaxIters, ISO_ERR_INVALID,
              "%s: bad n / max_iters (max %d)", c.who, kSdfMaxIters);
  if (c.n == 0) return 1;
  ISO_REQUIRE(c.n < (1ll << 31), ISO_ERR_UNSUPPORTED, "%s: n must fit int32", c.who);
  ISO_REQUIRE(ptrs_ok, ISO_ERR_INVALID, "%s: null pointer", c.who);
  return ISO_OK;
}

struct SdfLists { int32_t* idxA; int32_t* idxB; int32_t* counts; };   // counts: zero when the first launch starts

// Fills the call's fields of a family's argument block (SirenArgs / IdrArgs: same field names; the network's own fields
// are the family's) and runs launch(a, it) for it = 0 .. max_iters, once for an evaluation.  launch does what the family
// does around a launch -- tile counters, the kernel of its form -- and returns ISO_OK to go on, a negative error code, or
// kSdfStop when it has served every remaining iteration itself.
constexpr int kSdfStop = 1;
template <class Args, class Launch>
int sdf_run(const SdfCall& c, Args& a, const SdfLists& l, hipStream_t s, Launch&& launch) {
  a.n = c.n; a.tol = c.tol;
  a.fwd_only = c.value_only() ? 1 : 0;
  if (c.eval_only) {
    a.pts = const_cast<float*>(c.pts_in); a.normals = nullptr; a.mask = nullptr;
    a.sdf_out = c.sdf_out; a.grad_out = c.grad_out;
    a.idx_in = nullptr; a.count_in = nullptr; a.idx_out = nullptr; a.count_out = nullptr;
    a.do_move = 0; a.eval_only = 1;
    if (const int rc = launch(a, 0); rc < 0) return rc;
  } else {
    if (c.pts_out != c.pts_in) (void)hipMemcpyAsync(c.pts_out, c.pts_in, (size_t)c.n * 12, hipMemcpyDeviceToDevice, s);
    a.pts = c.pts_out; a.normals = c.normals_out; a.mask = c.mask_out; a.sdf_out = c.trace() ? c.sdf_out : nullptr;
    a.grad_out = nullptr; a.eval_only = 0;
    if (c.trace()) {                     // levelset_sampling.py:764,790: still active above 0.1 tol, valid up to tol
      a.dirs = c.dirs; a.alpha = c.alpha; a.bound = c.bound;
      a.tol = 0.1f * c.tol; a.tol_valid = c.tol;
    }
    for (int it = 0; it <= c.max_iters; ++it) {
      a.idx_in = (it == 0) ? nullptr : ((it & 1) ? l.idxA : l.idxB);
      a.count_in = (it == 0) ? nullptr : l.counts + it;
      a.idx_out = (it & 1) ? l.idxB : l.idxA;
      a.count_out = l.counts + it + 1;
      a.do_move = (it < c.max_iters) ? 1 : 0;
      const int rc = launch(a, it);
      if (rc < 0) return rc;
      if (rc == kSdfStop) break;
    }
  }
  ISO_CHECK_LAUNCH(c.who);
  return ISO_OK;
}
