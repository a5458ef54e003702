"""Every kernel form of the fused SIREN SDF path (csrc/siren_f32.hip, csrc/siren_x3.hip: five kernels in eighteen template
instances, picked by siren_form in csrc/siren.hip from hidden width, depth, value-only, codedness, the GEMM mode and the
step form) against the float64 oracle: each form at the depths no other test launches (n_hidden 0, 1, 5, 8), clouds that
end inside a tile, take a second round of workgroups and fall on either side of siren_split_point's 2 * 8192 rule, the
Newton loop with its one-launch tail at depths other than 3, sphere tracing on the value-only forms at depth 8, and one
latent-coded network per coded kernel instance at depth 5.

Every case first asserts iso_siren_step_kernel for the gradient and the value-only call: a re-dispatch fails here and not
by silently testing another kernel.  CASES / PROJECTED are also read by tests/test_siren_forms_cpu.py, which checks without
a GPU that they reach every k_siren_step* / k_siren_tail* kernel of the built library.

The criterion is SIREN's standing margin of test_projection_gpu.py::test_siren_grad_accuracy_vs_float64: with
e = max |grad - grad_float64|, m its mean and s the same max on the value, e_hip <= 2 e_ref + 1e-6, m_hip <= 1.5 m_ref + 1e-8
and s_hip <= 2 s_ref + 1e-7, the _ref figures being torch's float32 path on the same network and the whole cloud; plus
rel_err < 1e-5 (value) / 2e-5 (gradient) against that float32 path, the pair of tests/test_idr_forms_gpu.py (two
independent float32 paths at depth 8 lie within about 5e-6 of each other on the gradient).  The networks are the oracle's
SirenSDF at its default initialisation under a fixed seed: nothing is fitted."""
import copy
import functools

import pytest
import torch

from util import cube_cloud, fitted_siren, sphere_cloud

pytestmark = pytest.mark.gpu

MODES = {"split16": 1, "f32": 0}

# (hidden, n_hidden, mode, step form, code with gradient, code value-only)
# (a) each form at the depths nobody launches
FORMS = [(256, L, "split16", 1, 416, 216) for L in (1, 4, 5, 8)] + \
        [(256, L, "split16", 1, 516, 216) for L in (2, 3)] + \
        [(256, L, "split16", 0, 416, 216) for L in (2, 3)] + \
        [(128, L, "split16", 1, 308, 208) for L in (1, 5, 8)] + \
        [(64, L, "split16", 1, 104, 104) for L in (0, 8)] + \
        [(256, 0, "split16", 1, 116, 116), (128, 0, "split16", 1, 108, 108),
         (256, 8, "f32", 1, 116, 116), (128, 8, "f32", 1, 108, 108), (64, 5, "f32", 1, 104, 104)]
# (b) ragged ends and a second round: (case, points per workgroup P, workgroups of a round, value only)
RAGGED = [
    ((64, 2, "f32", 1, 104, 104), 64, 512, False),
    ((256, 2, "f32", 1, 116, 116), 64, 512, False),
    ((128, 2, "split16", 1, 308, 208), 96, 256, False),
    ((256, 2, "split16", 1, 516, 216), 96, 256, True),
]
# ... and the split list of 416 / 516: around siren_split_point (big = 256 * 96, small = 256 * 32)
SPLIT = [(256, 4, "split16", 1, 416, 216), (256, 3, "split16", 1, 516, 216)]
SPLIT_LONG = (24576, 24577, 24576 + 16384, 24576 + 16385)
SPLIT_SHORT = (1, 31, 32, 33, 95, 96, 97)
# (c) the Newton loop and its tail; the last two are launch-per-iteration controls (no tail kernel)
NEWTON = [(256, 1, "split16", 1, 416, 216), (256, 2, "split16", 1, 516, 216), (256, 4, "split16", 1, 416, 216),
          (256, 8, "split16", 1, 416, 216), (128, 8, "split16", 1, 308, 208), (256, 8, "f32", 1, 116, 116)]
NEWTON_SIZES = (999, 24673)
NEWTON_T = 6
# (d) sphere tracing on the value-only forms: (case, seed of a network on which some reference rays converge)
TRACE = [((256, 8, "split16", 1, 416, 216), 10), ((128, 8, "split16", 1, 308, 208), 1), ((64, 8, "split16", 1, 104, 104), 5),
         ((256, 8, "f32", 1, 116, 116), 10)]
# (e) one coded case per coded kernel instance: k_siren_step<4|8|16, 1>, k_siren_step_x3<128, .., 0|1, 1>,
# k_siren_step_x3<256, .., 1, 1>, k_siren_step_x3_both<.., 1> (and k_siren_tail_x3<.., 1> by the H = 256 projection)
CODED = [(64, 5, "split16", 1, 104, 104), (128, 5, "f32", 1, 108, 108), (256, 5, "f32", 1, 116, 116),
         (128, 5, "split16", 1, 308, 208), (256, 5, "split16", 1, 416, 216)]


def _rows(cases, value_only, coded):
    return [(c[0], c[1], v, coded, c[2], c[3], c[4 + v]) for c in cases for v in value_only]


# every (H, L, value_only, coded, mode, step form, expected code) a test of this file launches: all evaluate with and
# without the gradient, except the value-only ragged case, the Newton cases (gradient only) and the tracer's (value only)
CASES = _rows(FORMS + [r[0] for r in RAGGED if not r[3]] + SPLIT, (0, 1), 0) + _rows([r[0] for r in RAGGED if r[3]], (1,), 0) + \
        _rows(NEWTON, (0,), 0) + _rows([t[0] for t in TRACE], (1,), 0) + _rows(CODED, (0, 1), 1)
# the gradient cases a test of this file takes through a T = 6 projection: (H, L, coded, mode, step form, code)
PROJECTED = [(c[0], c[1], 0, c[2], c[3], c[4]) for c in NEWTON] + [(c[0], c[1], 1, c[2], c[3], c[4]) for c in CODED if c[4] // 100 == 4]


def _id(c):
    return "%dx%d-%s-form%d" % (c[1], c[0], c[2], c[3])


def _O():
    from oracle import iso_oracle as O
    return O


def _lib():
    from iso_points_amd import _lib as L
    return L.load()


@pytest.fixture
def knobs():
    """Sets the GEMM mode and the step form of a case (tests/test_siren_forms_cpu.py::knobs is the model); what was found is
    restored, and the Newton tail and the drawn tiles go back to their defaults."""
    lib = _lib()
    mode, form = lib.iso_siren_get_gemm_mode(), lib.iso_siren_get_step_form()

    def set_knobs(case):
        assert lib.iso_siren_set_gemm_mode(MODES[case[2]]) == 0 and lib.iso_siren_set_step_form(case[3]) == 0
        assert lib.iso_siren_get_gemm_mode() == MODES[case[2]] and lib.iso_siren_get_step_form() == case[3]
    yield set_knobs
    assert lib.iso_siren_set_gemm_mode(mode) == 0 and lib.iso_siren_set_step_form(form) == 0
    assert lib.iso_siren_set_tail_from(-1) == 0 and lib.iso_siren_set_drawn_tiles(-1) == 0


def _assert_codes(case, coded=0):
    """Under the knobs already set: the two kernels the case is meant to reach."""
    lib = _lib()
    H, L = case[:2]
    got = (lib.iso_siren_step_kernel(H, L, 0, coded), lib.iso_siren_step_kernel(H, L, 1, coded))
    assert got == (case[4], case[5]), (case, coded, got)


@functools.lru_cache(maxsize=None)
def _network(H, L, seed=None):
    """The oracle's SirenSDF at its default initialisation; shared (on the CPU, never modified)."""
    m = fitted_siren(_O(), H, L, seed=H + L if seed is None else seed, fit=0)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _reference_at(m, pts):
    """(network, points (n,3), float32 value and gradient by torch, the same in float64 on a .double() deep copy)"""
    O = _O()
    sdf32, grad32 = O.compute_sdf_and_grad(pts, m)
    sdf64, grad64 = O.compute_sdf_and_grad(pts.double(), copy.deepcopy(m).double())
    return m, pts, sdf32.reshape(-1), grad32, sdf64.reshape(-1), grad64


@functools.lru_cache(maxsize=None)
def _reference(H, L, n, seed):
    """The reference tuple on n points of the cube: made once per shape and cloud, shared by the modes and step forms."""
    return _reference_at(_network(H, L), cube_cloud(n, seed=seed)[0])


MEAN_FROM = 500


def _assert_margin(what, sdf, grad, ref, n=None):
    """The standing margin on ref's points, or on the first n of them; the measured figures are printed before they are
    judged.  e_ref, m_ref, s_ref and the scale of the relative errors are always the whole reference cloud's: a prefix of a
    few points is held to the cloud's margin, not to one relative to its own (possibly tiny) values.  The mean is judged
    on every whole cloud, and on a prefix of MEAN_FROM points or more; the mean error over a prefix of one or thirty
    points is no estimate of a cloud's (a single point's error is its own maximum, several times the cloud's mean), and
    such a prefix is held bit-equal to the rows of the long cloud, which is judged on the mean.  grad None: a value-only
    evaluation, judged on the value."""
    _, _, sdf32, grad32, sdf64, grad64 = ref
    sl = slice(None) if n is None else slice(0, n)
    sdf = sdf.cpu().reshape(-1)
    assert bool(torch.isfinite(sdf).all()), what
    s_ref = (sdf32.double() - sdf64).abs().max().item()
    s_hip = (sdf.double() - sdf64[sl]).abs().max().item()
    r_sdf = (sdf.double() - sdf32[sl].double()).abs().max().item() / sdf32.abs().max().item()
    if grad is None:
        print("%s: s_ref %.3g s_hip %.3g | rel vs f32: sdf %.3g" % (what, s_ref, s_hip, r_sdf))
        assert s_hip <= 2.0 * s_ref + 1e-7 and r_sdf < 1e-5, (what, s_ref, s_hip, r_sdf)
        return
    grad = grad.cpu()
    assert bool(torch.isfinite(grad).all()), what
    d_ref, d_hip = (grad32.double() - grad64).abs(), (grad.double() - grad64[sl]).abs()
    e_ref, e_hip, m_ref, m_hip = d_ref.max().item(), d_hip.max().item(), d_ref.mean().item(), d_hip.mean().item()
    r_grad = (grad.double() - grad32[sl].double()).abs().max().item() / grad32.abs().max().item()
    print("%s: e_ref %.3g e_hip %.3g m_ref %.3g m_hip %.3g s_ref %.3g s_hip %.3g | rel vs f32: sdf %.3g grad %.3g"
          % (what, e_ref, e_hip, m_ref, m_hip, s_ref, s_hip, r_sdf, r_grad))
    assert e_hip <= 2.0 * e_ref + 1e-6 and s_hip <= 2.0 * s_ref + 1e-7, (what, e_ref, e_hip, s_ref, s_hip)
    if n is None or n >= MEAN_FROM:
        assert m_hip <= 1.5 * m_ref + 1e-8, (what, m_ref, m_hip)
    assert r_sdf < 1e-5 and r_grad < 2e-5, (what, r_sdf, r_grad)


def _evaluate(pk, m, pts, code=None, value_only=False):
    """Value and gradient, then value only: the rule of test_trace_gpu.py::test_value_only_evaluation_equals_the_full_one, at
    every case (not a bit of the value may change when the reverse sweep is skipped, also where another kernel serves
    the value: the forward sweeps of 308 / 208 and of 416 / 516 / 216 are one text)."""
    from iso_points_amd.sdf_models import siren_sdf_and_grad
    val, none = siren_sdf_and_grad(m, pts, need_grad=False, packed=pk, code=code)
    assert none is None and val.shape == pts.shape[:1]
    if value_only:
        return val, None
    sdf, grad = siren_sdf_and_grad(m, pts, packed=pk, code=code)
    assert sdf.shape == pts.shape[:1] and grad.shape == pts.shape
    assert torch.equal(val, sdf), int((val != sdf).sum())
    return sdf, grad


def _packed(m, dev):
    from iso_points_amd.sdf_models import PackedSiren
    return PackedSiren(m, dev)


# ---- (a) each form at the depths nobody launches --------------------------------------------------------------------------
@pytest.mark.parametrize("case", FORMS, ids=_id)
def test_every_form_and_depth_against_float64(dev, knobs, case):
    """1 500 points of the cube: value and gradient, then value only.  Depth 8 is what include/isopoints.h promises: the
    (L + 1)-slot stash of the f32 kernel, the L-slot one of the split-fp16 kernels, the header slots [l] and [8 + l] and
    the per-point adjoint scale, whose bound compounds layer by layer, at their last index."""
    knobs(case)
    _assert_codes(case)
    H, L = case[:2]
    ref = _reference(H, L, 1500, L)
    m, pts = ref[0], ref[1].to(dev)
    sdf, grad = _evaluate(_packed(m, dev), m, pts)
    _assert_margin("%s codes %d/%d" % (_id(case), case[4], case[5]), sdf, grad, ref)


# ---- (b) ragged ends, more than one round ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,per_wg,wgs,value_only", RAGGED, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_ragged_ends_and_second_round(dev, knobs, case, per_wg, wgs, value_only):
    """A round of the grid plus a tile and a point (every workgroup takes a second tile or ends, the last one ragged), whole,
    under the margin; then its first n points for n = 1, one tile less a point, one tile, one tile and a point, under the
    same margin and bit-equal to the long result's first n rows: a point's evaluation does not depend on the tile it sits
    in (include/isopoints.h).  216 is evaluated value only: its gradient partner at this shape is 516, of the next test."""
    knobs(case)
    _assert_codes(case)
    H, L = case[:2]
    n_long = wgs * per_wg + per_wg + 1
    ref = _reference(H, L, n_long, 7)
    m, pts = ref[0], ref[1].to(dev)
    pk = _packed(m, dev)
    sdf, grad = _evaluate(pk, m, pts, value_only=value_only)
    _assert_margin("%s n=%d" % (_id(case), n_long), sdf, grad, ref)
    for n in (1, per_wg - 1, per_wg, per_wg + 1):
        s, g = _evaluate(pk, m, pts[:n].contiguous(), value_only=value_only)
        _assert_margin("%s n=%d" % (_id(case), n), s, g, ref, n)
        assert torch.equal(s, sdf[:n]) and (value_only or torch.equal(g, grad[:n])), n


@pytest.mark.parametrize("case", SPLIT, ids=_id)
def test_split_list_on_both_sides_of_the_split_point(dev, knobs, case):
    """416 / 516 cut a list at siren_split_point into 96-point and 32-point tiles: no remainder (24 576), a remainder of one
    point, a remainder that just fits two rounds of the small tiles (16 384) and one that takes another round of the large
    ones (16 385); and the short lists around both tile sizes.  Every size is a prefix of the longest cloud: each under the
    margin against the one reference and bit-equal to the longest result's first n rows, with drawn tiles and with static
    shares (iso_siren_set_drawn_tiles 1 / 0), whose results are bit-identical."""
    knobs(case)
    _assert_codes(case)
    lib = _lib()
    H, L = case[:2]
    n_max = max(SPLIT_LONG)
    ref = _reference(H, L, n_max, 7)
    m, pts = ref[0], ref[1].to(dev)
    pk = _packed(m, dev)
    per_setting = []
    for drawn in (1, 0):
        assert lib.iso_siren_set_drawn_tiles(drawn) == 0
        sdf, grad = _evaluate(pk, m, pts)
        _assert_margin("%s n=%d drawn=%d" % (_id(case), n_max, drawn), sdf, grad, ref)
        outs = [sdf, grad]
        for n in SPLIT_SHORT + SPLIT_LONG[:-1]:
            s, g = _evaluate(pk, m, pts[:n].contiguous())
            _assert_margin("%s n=%d drawn=%d" % (_id(case), n, drawn), s, g, ref, n)
            assert torch.equal(s, sdf[:n]) and torch.equal(g, grad[:n]), (n, drawn)
            outs += [s, g]
        per_setting.append(outs)
    for a, b in zip(*per_setting):
        assert torch.equal(a, b)


# ---- (c) the Newton loop and its one-launch tail ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _newton_reference(H, L, n):
    """(network, start points (1,n,3), tolerance, the float32 oracle's projection with T = 6 and with T = 1, the float32
    and float64 start values).  A default-initialised SIREN is no SDF, so the tolerance comes from the reference: the 0.3
    quantile of |f| over the float32 oracle's values at the start points -- then the lists do shrink and do not die out."""
    O = _O()
    m = _network(H, L)
    pts = sphere_cloud(n, seed=n) * 0.9
    start = _reference_at(m, pts[0])
    tol = float(torch.quantile(start[2].abs(), 0.3))
    num = torch.tensor([n])
    ref6 = O.project_points(m, pts, num, proj_max_iters=NEWTON_T, proj_tolerance=tol)
    ref1 = O.project_points(m, pts, num, proj_max_iters=1, proj_tolerance=tol)
    at_start, after = int((start[2].abs() <= tol).sum()), int(ref6.mask.sum())
    assert at_start < after < n, (at_start, after, n)           # (conditions on the reference alone)
    return m, pts, tol, ref6, ref1, start


def _project(dev, m, x, T, tol, tail_from, **kw):
    """-> (ProjectionResult, the per-iteration counts [1 .. T] the projection leaves in its workspace)"""
    from iso_points_amd.levelset_sampling import UniformProjection, full_lengths
    lib = _lib()
    lengths = kw.pop("lengths", None)
    n = int(x.shape[0] * x.shape[1]) if lengths is None else int(sum(lengths))
    proj = UniformProjection(proj_tolerance=tol)
    assert lib.iso_siren_set_tail_from(tail_from) == 0
    r = proj._project_points(m, x, full_lengths(x) if lengths is None else torch.tensor(lengths, device=dev),
                             proj_max_iters=T, **kw)
    torch.cuda.synchronize()
    pk = proj._packed_cache
    off = lib.iso_project_siren_counts_offset(n, pk.hidden, pk.n_hidden)
    return r, pk._ws[off:off + 64 * 4].view(torch.int32)[1:T + 1].tolist()


def _assert_tail_equals_launch_per_iteration(dev, m, x, n, T, tol, **kw):
    """The method of test_round4_gpu.py::test_newton_tail_in_one_launch_equals_a_launch_per_iteration: points, normals, mask
    and the per-iteration counts of iso_siren_set_tail_from(0) against -1 (the default), 1, 2 and T, bit for bit; the
    counts are the counters (non-increasing) and the lists did shrink."""
    ref, c_ref = _project(dev, m, x, T, tol, 0, **kw)
    print("counts %s of %d" % (c_ref, n))
    assert all(a >= b for a, b in zip(c_ref, c_ref[1:])) and 0 < c_ref[0] < n, (c_ref, n)
    for k in (-1, 1, 2, T):
        out, c = _project(dev, m, x, T, tol, k, **kw)
        assert torch.equal(out.points, ref.points) and torch.equal(out.normals, ref.normals) and \
            torch.equal(out.mask, ref.mask), k
        assert c == c_ref, (k, c, c_ref)
    return ref


UNDECIDED_CAP = 0.01


@pytest.mark.parametrize("n", NEWTON_SIZES)
@pytest.mark.parametrize("case", NEWTON, ids=_id)
def test_newton_loop_and_tail_at_other_depths(dev, knobs, case, n):
    """T = 6 from sphere_cloud(n) * 0.9 at the reference's own tolerance.
    1. the tail against a launch per iteration, bit for bit, from every iteration it may start at (128 x 8 and the f32 mode
       have no tail kernel: there the settings must change nothing at all);
    2. against float64, independent of the chaotic trajectory: a point is last evaluated where it ends, so the normals ARE
       the kernel's gradient at its own final positions (held to the margin there, e_ref being torch's float32 gradient at
       those positions) and the mask is |f| <= tol, equal to the float64 value's wherever that is further from the
       tolerance than the margin on the value (at most 1 % of the points may be nearer);
    3. one move is not chaotic: after T = 1 every point whose start value is decided in that sense lies within 1e-5
       (relative to the largest coordinate) of the float32 oracle's."""
    knobs(case)
    _assert_codes(case)
    H, L = case[:2]
    m, pts, tol, ref6, ref1, start = _newton_reference(H, L, n)
    x = pts.to(dev)
    res = _assert_tail_equals_launch_per_iteration(dev, m, x, n, NEWTON_T, tol)
    # 2.
    at_end = _reference_at(m, res.points.cpu()[0])
    normals, mask = res.normals.cpu()[0], res.mask.cpu()[0]
    s_ref = (at_end[2].double() - at_end[4]).abs().max().item()
    decided = (at_end[4].abs() - tol).abs() > 2.0 * s_ref + 1e-7
    print("%s n=%d tol %.4g: %d converged (oracle %d), undecided share %.5f of cap %g" % (
        _id(case), n, tol, int(mask.sum()), int(ref6.mask.sum()), 1.0 - decided.float().mean().item(), UNDECIDED_CAP))
    # (the projection returns no value: the reference's own float32 value stands in for it, only the gradient is judged)
    _assert_margin("%s n=%d normals at the end points" % (_id(case), n), at_end[2], normals, at_end)
    assert 1.0 - decided.float().mean().item() <= UNDECIDED_CAP
    assert torch.equal(mask[decided], (at_end[4].abs() <= tol)[decided])
    # 3.
    one, _ = _project(dev, m, x, 1, tol, -1)
    s_ref0 = (start[2].double() - start[4]).abs().max().item()
    decided0 = (start[4].abs() - tol).abs() > 2.0 * s_ref0 + 1e-7
    err = (one.points.cpu()[0].double() - ref1.points[0].double()).abs().amax(-1) / ref1.points.abs().max().item()
    print("%s n=%d T=1: max rel position error %.3g on the decided points, undecided share %.5f" % (
        _id(case), n, err[decided0].max().item(), 1.0 - decided0.float().mean().item()))
    assert 1.0 - decided0.float().mean().item() <= UNDECIDED_CAP
    assert err[decided0].max().item() <= 1e-5


# ---- (d) sphere tracing on the value-only forms at depth 8 -----------------------------------------------------------------
@pytest.mark.parametrize("case,seed", TRACE, ids=lambda v: _id(v) if isinstance(v, tuple) else "seed%d" % v)
def test_trace_at_depth_eight(dev, knobs, case, seed):
    """SphereTracing (value only inside the loop) under the rule of test_trace_gpu.py::test_trace_siren_vs_oracle, at its
    tolerances (1e-5 on the positions, stop_tol 1e-4: a default-initialised SIREN is not 1-Lipschitz), on 1 500 rays and
    eight iterations as tests/test_idr_forms_gpu.py traces.  The seeds are those for which some rays of the reference both
    stay inside the bound and converge (most default initialisations have no zero on these rays: asserted here)."""
    O = _O()
    from iso_points_amd.levelset_sampling import SphereTracing
    from test_oracle_golden import assert_trace_close
    from test_trace_gpu import _rays
    knobs(case)
    _assert_codes(case)
    m = _network(case[0], case[1], seed)
    r0, d = _rays(1500, 22, dev)
    ref = O.sphere_trace(m, r0, d, proj_max_iters=8)
    inside = ref["levelset_points"].norm(dim=-1) < 1.1
    print("%s: %d of 1500 reference rays converged inside the bound" % (_id(case), int((ref["mask"] & inside).sum())))
    assert int((ref["mask"] & inside).sum()) > 0 and int((~ref["mask"]).sum()) > 0
    out = SphereTracing(proj_max_iters=8).project_points(r0.to(dev), d.to(dev), m)
    assert_trace_close(out, ref["levelset_points"], ref["network_eval_on_levelset_points"], ref["mask"], tol=1e-5, stop_tol=1e-4)


# ---- (e) one coded case per coded kernel instance ----------------------------------------------------------------------------
class _WithCode(torch.nn.Module):
    """The coded model's own torch forward with each point's code concatenated: what the oracle differentiates."""

    def __init__(self, m, rows):
        super().__init__()
        self.m, self.rows = m, rows

    def forward(self, x, **kw):
        return self.m(x, c=self.rows)


@functools.lru_cache(maxsize=None)
def _coded_reference(H, L):
    """(Siren(c_dim = 8), two codes, code_of, the reference tuple of its 197 points)"""
    from iso_points_amd.sdf_models import Siren
    n, C = 197, 8
    torch.manual_seed(H + L)
    m = Siren(hidden_size=H, n_layers=L, c_dim=C)
    for p in m.parameters():
        p.requires_grad_(False)
    codes = torch.randn(2, C, generator=torch.Generator().manual_seed(2))
    code_of = (torch.arange(n) >= 100).to(torch.int32)
    pts = sphere_cloud(n, seed=5)[0] * 0.9
    O = _O()
    rows = codes[code_of.long()]
    sdf32, grad32 = O.compute_sdf_and_grad(pts, _WithCode(m, rows))
    sdf64, grad64 = O.compute_sdf_and_grad(pts.double(), _WithCode(copy.deepcopy(m).double(), rows.double()))
    return m, codes, code_of, (m, pts, sdf32.reshape(-1), grad32, sdf64.reshape(-1), grad64)


@pytest.mark.parametrize("case", CODED, ids=_id)
def test_coded_network_per_coded_kernel(dev, knobs, case):
    """Siren(c_dim = 8) of five hidden layers (tests/test_latent_gpu.py stops at three), two codes over 197 points: value and
    gradient under the margin, the reference being the model's own forward with the code concatenated, in float32 and
    float64.  H = 256, split-fp16: a T = 6 coded projection, its tail (k_siren_tail_x3<.., 1>) against a launch per
    iteration, bit for bit."""
    from iso_points_amd.sdf_models import CodeRows
    knobs(case)
    _assert_codes(case, coded=1)
    H, L = case[:2]
    m, codes, code_of, ref = _coded_reference(H, L)
    pts = ref[1].to(dev)
    code = CodeRows(codes.to(dev), code_of.to(dev))
    sdf, grad = _evaluate(_packed(m, dev), m, pts, code=code)
    _assert_margin("%s coded, codes %d/%d" % (_id(case), case[4], case[5]), sdf, grad, ref)
    if case[4] // 100 == 4:                                     # (the cases PROJECTED lists)
        tol = float(torch.quantile(ref[2].abs(), 0.3))
        x = torch.zeros(2, 100, 3, device=dev)                  # two clouds, 100 and 97 points: a code each
        x[0], x[1, :97] = pts[:100], pts[100:]
        _assert_tail_equals_launch_per_iteration(dev, m, x, 197, NEWTON_T, tol, lengths=[100, 97], c=codes.to(dev))
