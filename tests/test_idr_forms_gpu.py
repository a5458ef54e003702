"""Every kernel form of the fused IDR SDF path (csrc/idr_f32.hip, csrc/idr_x16.hip: three kernels in twelve template
instances, picked by idr_form in csrc/idr.hip from hidden width, encoding width, value-only and the GEMM mode) against the
float64 oracle: each form once, the limits of the accepted shapes, clouds that end inside a tile and take more than one
round of workgroups, the Newton loop and the tracer on the forms no other test enters, a mode switch between two calls
on one packed model, and 130 points through each family's launch entry at H = 256 and 512.

Every case first asserts iso_idr_step_form: a re-dispatch fails here and not by silently testing another kernel.  CASES
is also read by tests/test_idr_forms_cpu.py, which checks without a GPU that it reaches every k_idr_step* kernel of the
built library.

The criterion is the one of test_idr_gpu.py::test_idr_shapes_vs_oracle_and_float64: with e = max |x - x_float64|,
e_hip <= 1.5 e_ref + 2e-6 on the gradient and s_hip <= 1.5 s_ref + 2e-7 on the value, e_ref / s_ref being torch's
float32 path on the same network, plus rel_err < 1e-5 (value) / 2e-5 (gradient) against that float32 path."""
import copy
import functools

import pytest
import torch

from util import assert_projection_close, cube_cloud, rel_err, sphere_cloud

pytestmark = pytest.mark.gpu

MODES = {"split16": 1, "f32": 0}

# (hidden, n_layers, skip (-1: none), n_freq, mode, form with gradient, form value-only)
# (a) each form the other tests never launch, once
FORMS = [
    (512, 3, 2, 6, "f32", 232, 332),
    (256, 3, 1, 6, "f32", 216, 316),
    (512, 3, -1, 7, "split16", 232, 332),
    (256, 4, 3, 7, "split16", 216, 316),
    (512, 3, 1, 8, "split16", 132, 132),
    (512, 2, -1, 10, "split16", 132, 132),
    (256, 3, -1, 9, "split16", 116, 116),
    (128, 3, 2, 10, "split16", 108, 108),
    (128, 2, -1, 7, "split16", 108, 308),
]
# (b) the limits idr_shape_ok accepts -- 2 and 12 layers; skip at 1, at n_layers - 1, none; no frequencies -- on the
# split-fp16 form and on one f32 form each
LIMITS = [
    (512, 2, 1, 6, "split16", 432, 532),
    (256, 2, -1, 0, "split16", 416, 516),
    (256, 12, 11, 4, "split16", 416, 516),
    (512, 12, 1, 0, "split16", 432, 532),
    (512, 2, -1, 0, "f32", 232, 332),
    (256, 2, 1, 6, "f32", 216, 316),
    (256, 12, 1, 2, "f32", 216, 316),
    (256, 12, 11, 7, "split16", 216, 316),
    (128, 12, 11, 8, "split16", 108, 108),
]
# (c) ragged ends and a second round of workgroups, per family, two-layer networks: (case, points per workgroup)
RAGGED = [
    ((512, 2, -1, 6, "f32", 232, 332), 64),
    ((256, 2, 1, 8, "split16", 116, 116), 64),
    ((512, 2, 1, 6, "split16", 432, 532), 64),
    ((256, 2, -1, 6, "split16", 416, 516), 96),
]
# (d) the Newton loop and the tracer
NEWTON = [
    (256, 4, 2, 6, "f32", 216, 316),
    (512, 3, 2, 7, "split16", 232, 332),
    (256, 3, 1, 9, "split16", 116, 116),
    (512, 3, 2, 8, "split16", 132, 132),
]
TRACE = [
    (256, 4, 2, 6, "f32", 216, 316),
    (512, 3, 2, 6, "f32", 232, 332),
    (512, 3, 2, 8, "split16", 132, 132),
]
# (f) the two launch entries (idr_f32_launch, idr_x16_launch) at both widths either serves: 130 points
BOUNDARY = [
    (256, 3, 1, 6, "split16", 416, 516),
    (512, 3, 2, 6, "split16", 432, 532),
    (256, 3, 1, 6, "f32", 216, 316),
    (512, 3, 2, 6, "f32", 232, 332),
]
# every (case, value_only) pair a test of this file launches: all of them evaluate with and without the gradient, except
# the Newton cases (gradient only) and the tracer's (value only)
CASES = [(c, v) for c in FORMS + LIMITS + [r[0] for r in RAGGED] + BOUNDARY for v in (0, 1)] + [(c, 0) for c in NEWTON] + \
        [(c, 1) for c in TRACE]


def _id(c):
    return "%dx%d-skip%s-F%d-%s" % (c[1], c[0], c[2] if c[2] >= 0 else "no", c[3], c[4])


def _O():
    from oracle import iso_oracle as O
    return O


@pytest.fixture
def idr_mode():
    """Sets the IDR GEMM mode (include/isopoints.h: iso_idr_set_gemm_mode) by name; the mode found is restored."""
    from iso_points_amd import _lib
    lib = _lib.load()
    before = lib.iso_idr_get_gemm_mode()

    def set_mode(name):
        _lib.call("iso_idr_set_gemm_mode", MODES[name])
        assert lib.iso_idr_get_gemm_mode() == MODES[name]
    yield set_mode
    _lib.call("iso_idr_set_gemm_mode", before)
    lib.iso_idr_set_drawn_tiles(-1)


def _assert_forms(case):
    """Under the mode already set: the two forms the case is meant to reach."""
    from iso_points_amd import _lib
    H, NL, skip, F, mode, form_grad, form_value = case
    lib = _lib.load()
    got = (lib.iso_idr_step_form(H, NL, skip, F, 0), lib.iso_idr_step_form(H, NL, skip, F, 1))
    assert got == (form_grad, form_value), (case, got)


def _network(case, perturb=True):
    H, NL, skip, F = case[:4]
    torch.manual_seed(H + NL)
    m = _O().IdrSDF(hidden_size=H, n_layers=NL, skip_in=(skip,) if skip >= 0 else (), num_frequencies=F)
    if perturb:
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01 * torch.randn_like(p))
    for p in m.parameters():
        p.requires_grad_(False)
    return m


@functools.lru_cache(maxsize=None)
def _reference(case, n, seed):
    """(network, points (n,3), float32 value and gradient by torch, the same in float64): made once per case."""
    O = _O()
    m = _network(case)
    pts = cube_cloud(n, seed=seed)[0]
    sdf32, grad32 = O.compute_sdf_and_grad(pts, m)
    sdf64, grad64 = O.compute_sdf_and_grad(pts.double(), copy.deepcopy(m).double())
    return m, pts, sdf32, grad32, sdf64, grad64


def _assert_margin(what, sdf, grad, ref, sl=slice(None)):
    """The standing parity margin on ref's points [sl]; the measured figures are printed before they are judged.  e_ref,
    s_ref and the scale of the relative errors are always the whole reference cloud's: a prefix of a few points is held to
    the cloud's margin, not to one relative to its own (possibly tiny) values."""
    _, _, sdf32, grad32, sdf64, grad64 = ref
    sdf, grad = sdf.cpu(), grad.cpu()
    assert bool(torch.isfinite(sdf).all()) and bool(torch.isfinite(grad).all()), what
    e_ref = (grad32.double() - grad64).abs().max().item()
    e_hip = (grad.double() - grad64[sl]).abs().max().item()
    s_ref = (sdf32.double() - sdf64).abs().max().item()
    s_hip = (sdf.double() - sdf64[sl]).abs().max().item()
    r_sdf = (sdf.double() - sdf32[sl].double()).abs().max().item() / sdf32.abs().max().item()
    r_grad = (grad.double() - grad32[sl].double()).abs().max().item() / grad32.abs().max().item()
    print("%s: e_ref %.3g e_hip %.3g s_ref %.3g s_hip %.3g | rel vs f32: sdf %.3g grad %.3g"
          % (what, e_ref, e_hip, s_ref, s_hip, r_sdf, r_grad))
    assert e_hip <= 1.5 * e_ref + 2e-6 and s_hip <= 1.5 * s_ref + 2e-7, (what, e_ref, e_hip, s_ref, s_hip)
    assert r_sdf < 1e-5 and r_grad < 2e-5, (what, r_sdf, r_grad)


def _evaluate(case, pk, m, pts):
    """Value and gradient, then value only: the rule of test_trace_gpu.py::test_value_only_evaluation_equals_the_full_one
    (not a bit may change -- except where the two run different kernels: H = 128 takes the staged kernel for the gradient
    and the feature-split one for the value, whose sums run in another order)."""
    from iso_points_amd.sdf_models import idr_sdf_and_grad
    sdf, grad = idr_sdf_and_grad(m, pts, packed=pk)
    val, none = idr_sdf_and_grad(m, pts, need_grad=False, packed=pk)
    assert none is None
    if (case[5], case[6]) == (108, 308):
        assert rel_err(val, sdf) < 1e-6
    else:
        assert torch.equal(val, sdf), (case, int((val != sdf).sum()))
    return sdf, grad


def _check_case(dev, idr_mode, case, n=1500):
    from iso_points_amd.sdf_models import PackedIdr
    idr_mode(case[4])
    _assert_forms(case)
    ref = _reference(case, n, case[1])
    m, pts = ref[0], ref[1]
    sdf, grad = _evaluate(case, PackedIdr(m, dev), m, pts.to(dev))
    _assert_margin("%s forms %d/%d" % (_id(case), case[5], case[6]), sdf, grad, ref)


# ---- (a) each form once ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FORMS, ids=_id)
def test_every_unlaunched_form_against_float64(dev, idr_mode, case):
    """1 500 points of the cube, the 0.01-perturbed network of test_idr_shapes_vs_oracle_and_float64: value and gradient, then
    value only.  8 x 512 with 8..10 frequencies is k_idr_step<32>, which asks for 163 840 B of LDS: all a workgroup can
    have."""
    _check_case(dev, idr_mode, case)


# ---- (b) the limits of the accepted shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LIMITS, ids=_id)
def test_shape_limits_against_float64(dev, idr_mode, case):
    """2 and 12 layers, the skip connection into layer 1 and into the last layer and none, no frequencies (D0 = 3: the
    encoding is the point), on the split-fp16 kernel and on one f32 kernel each."""
    _check_case(dev, idr_mode, case)


# ---- (c) ragged ends, more than one round --------------------------------------------------------------------------------
@pytest.mark.parametrize("case,per_wg", RAGGED, ids=lambda v: _id(v) if isinstance(v, tuple) else "wg%d" % v)
def test_ragged_ends_and_second_round(dev, idr_mode, case, per_wg):
    """n = 1, one tile less one point, one tile, one tile and a point, and 256 workgroups' tiles plus a tile and a point (the
    grid is 256 workgroups at most: every workgroup of the long cloud takes a second tile or ends, the last one ragged).
    The long cloud whole against float64; the short ones are its first n points, against the same reference.

    Bit checks: a point's arithmetic depends on its tile neighbours in none of the forms -- the f32 kernels by construction
    (a point is one column of the MFMA's B operand, the sums over features are per point and in a fixed order), and the
    split-fp16 kernel too: its power-of-two operand scales (bscale, nscale, zs, inv), the bounds Mp they come from and the
    maxima exchanged through LDS (redm) are all indexed by the point (32 n + j), the weight scales are the layer's, and
    the sums over the waves run in wave order.  So for EVERY family here the long cloud evaluated in slices of one round
    (256 tiles) must equal the one call bit for bit, and so must every short cloud equal the long one's first n points.
    The split-fp16 cases run with drawn tiles and with static shares (iso_idr_set_drawn_tiles 1 / 0): bit-identical."""
    from iso_points_amd import _lib
    from iso_points_amd.sdf_models import PackedIdr
    idr_mode(case[4])
    _assert_forms(case)
    lib = _lib.load()
    one_round = 256 * per_wg
    n_long = one_round + per_wg + 1
    ref = _reference(case, n_long, 7)
    m, pts = ref[0], ref[1].to(dev)
    pk = PackedIdr(m, dev)
    x16 = case[5] >= 400
    per_setting = []
    for drawn in ((1, 0) if x16 else (-1,)):
        assert lib.iso_idr_set_drawn_tiles(drawn) == 0
        sdf, grad = _evaluate(case, pk, m, pts)
        _assert_margin("%s n=%d drawn=%d" % (_id(case), n_long, drawn), sdf, grad, ref)
        parts = [_evaluate(case, pk, m, pts[a:a + one_round].contiguous()) for a in range(0, n_long, one_round)]
        assert torch.equal(torch.cat([p[0] for p in parts]), sdf) and torch.equal(torch.cat([p[1] for p in parts]), grad)
        shorts = []
        for n in (1, per_wg - 1, per_wg, per_wg + 1):
            s, g = _evaluate(case, pk, m, pts[:n].contiguous())
            assert s.shape == (n,) and g.shape == (n, 3)
            _assert_margin("%s n=%d drawn=%d" % (_id(case), n, drawn), s, g, ref, slice(0, n))
            assert torch.equal(s, sdf[:n]) and torch.equal(g, grad[:n]), n
            shorts += [s, g]
        per_setting.append([sdf, grad] + shorts)
    if x16:
        for a, b in zip(*per_setting):
            assert torch.equal(a, b)


# ---- (d) the Newton loop and the tracer on the new forms ---------------------------------------------------------------
@pytest.mark.parametrize("case", NEWTON, ids=_id)
def test_projection_on_the_new_forms(dev, idr_mode, case):
    """Geometric init ~ sphere of radius 0.6, 3 000 points, ten Newton iterations at the default tolerance (index lists,
    count_in / count_out): as test_idr_gpu.py::test_idr_projection_converges_like_oracle."""
    O = _O()
    from iso_points_amd.levelset_sampling import UniformProjection, full_lengths
    idr_mode(case[4])
    _assert_forms(case)
    m = _network(case, perturb=False)
    pts = sphere_cloud(3000, seed=2) * 0.6
    ref = O.project_points(m, pts, torch.tensor([3000]), proj_max_iters=10)
    x = pts.to(dev)
    res = UniformProjection()._project_points(m, x, full_lengths(x), proj_max_iters=10)
    assert_projection_close(res.points, ref.points)
    assert (res.mask.cpu() == ref.mask).float().mean() > 0.995
    assert ref.mask.float().mean() > 0.9


@pytest.mark.parametrize("case", TRACE, ids=_id)
def test_trace_on_the_new_forms(dev, idr_mode, case):
    """SphereTracing (fwd_only inside the loop) under the rule of test_trace_gpu.py::test_trace_idr_vs_oracle."""
    O = _O()
    from iso_points_amd.levelset_sampling import SphereTracing
    from test_oracle_golden import assert_trace_close
    from test_trace_gpu import _rays
    idr_mode(case[4])
    _assert_forms(case)
    m = _network(case, perturb=False)
    r0, d = _rays(1500, 22, dev)
    ref = O.sphere_trace(m, r0, d, proj_max_iters=8)
    out = SphereTracing(proj_max_iters=8).project_points(r0.to(dev), d.to(dev), m.to(dev))
    assert_trace_close(out, ref["levelset_points"], ref["network_eval_on_levelset_points"], ref["mask"], tol=2e-5)


# ---- (e) a mode switch between two calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(512, 3, 2, 6), (256, 4, 3, 4)], ids=lambda c: "%dx%d" % (c[1], c[0]))
def test_mode_switch_on_one_packed_model(dev, idr_mode, case):
    """One PackedIdr (packed once, one workspace): split-fp16, then f32, then split-fp16 again.  The packed buffer holds both
    images and the workspace is sized for both forms: the first and the third result are bit-identical, the second is
    within the margin."""
    from iso_points_amd.sdf_models import PackedIdr
    NT = case[0] // 16
    c16, c32 = case + ("split16", 400 + NT, 500 + NT), case + ("f32", 200 + NT, 300 + NT)
    ref = _reference(c16, 1500, 11)
    m, pts = ref[0], ref[1].to(dev)
    pk = PackedIdr(m, dev)
    outs = []
    for c in (c16, c32, c16):
        idr_mode(c[4])
        _assert_forms(c)
        sdf, grad = _evaluate(c, pk, m, pts)
        _assert_margin("%s after a switch" % _id(c), sdf, grad, ref)
        outs.append((sdf, grad))
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    assert not torch.equal(outs[0][1], outs[1][1])            # (the f32 kernels did run: another rounding)


# ---- (f) 130 points through each family's launch entry -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary_cloud(case):
    """(network at its geometric initialisation ~ a sphere of radius 0.6, 130 points around it, the float32 oracle's
    projection of them with three Newton iterations): made once per case."""
    m = _network(case, perturb=False)
    pts = sphere_cloud(130, seed=3) * 0.6
    return m, pts, _O().project_points(m, pts, torch.tensor([130]), proj_max_iters=3)


def _reference_at(m, pts):
    """_reference's tuple for given points (n,3)."""
    O = _O()
    sdf32, grad32 = O.compute_sdf_and_grad(pts, m)
    sdf64, grad64 = O.compute_sdf_and_grad(pts.double(), copy.deepcopy(m).double())
    return m, pts, sdf32, grad32, sdf64, grad64


@pytest.mark.parametrize("case", BOUNDARY, ids=_id)
def test_projection_of_130_points_per_family_and_width(dev, idr_mode, case):
    """130 points are two full 64-point tiles and a part tile (96 + 34 on k_idr_step_x16<256, 3>): three workgroups at
    most, four launches on the two index lists (max_iters = 3, default tolerance: some points stop early, so the lists
    shrink).  Positions against the float32 oracle's projection under assert_projection_close, as (d) does.  Against
    float64: a point is last evaluated where it ends (a launch that moves a point keeps it on the list, the last launch
    moves nothing), so the normals ARE the kernel's gradient at its own final positions and are held to the standing
    margin on the gradient there, e_ref being torch's float32 gradient at those positions; and the mask is |f| <= tol, so
    it must equal the float64 value's wherever that is further from the tolerance than the standing margin on the value."""
    from iso_points_amd.levelset_sampling import UniformProjection, full_lengths
    idr_mode(case[4])
    _assert_forms(case)
    m, pts, ref = _boundary_cloud(case)
    x = pts.to(dev)
    proj = UniformProjection()
    res = proj._project_points(m, x, full_lengths(x), proj_max_iters=3)
    assert_projection_close(res.points, ref.points)
    _, _, sdf32, grad32, sdf64, grad64 = _reference_at(m, res.points.cpu()[0])
    normals, mask = res.normals.cpu()[0], res.mask.cpu()[0]
    assert bool(torch.isfinite(normals).all())
    e_ref = (grad32.double() - grad64).abs().max().item()
    e_hip = (normals.double() - grad64).abs().max().item()
    r_grad = (normals.double() - grad32.double()).abs().max().item() / grad32.abs().max().item()
    s_ref = (sdf32.double() - sdf64).abs().max().item()
    decided = (sdf64.abs() - proj.proj_tolerance).abs() > 1.5 * s_ref + 2e-7
    print("%s projection: e_ref %.3g e_hip %.3g rel vs f32 %.3g | s_ref %.3g, %d of 130 converged, %d within the margin of "
          "the tolerance" % (_id(case), e_ref, e_hip, r_grad, s_ref, int(mask.sum()), int((~decided).sum())))
    assert e_hip <= 1.5 * e_ref + 2e-6 and r_grad < 2e-5, (e_ref, e_hip, r_grad)
    assert torch.equal(mask[decided], (sdf64.abs() <= proj.proj_tolerance)[decided])
    assert 0 < int(mask.sum())                                  # (the lists did shrink: some points stopped)


@pytest.mark.parametrize("case", BOUNDARY, ids=_id)
def test_evaluation_of_130_points_per_family_and_width(dev, idr_mode, case):
    """The same 130 points through iso_idr_sdf_grad with grad_out and without it (the gradient form and the value form of
    either entry), under the standing margin."""
    from iso_points_amd.sdf_models import PackedIdr
    idr_mode(case[4])
    _assert_forms(case)
    m, pts, _ = _boundary_cloud(case)
    ref = _reference_at(m, pts[0])
    sdf, grad = _evaluate(case, PackedIdr(m, dev), m, pts[0].to(dev))
    assert sdf.shape == (130,) and grad.shape == (130, 3)
    _assert_margin("%s n=130 forms %d/%d" % (_id(case), case[5], case[6]), sdf, grad, ref)
