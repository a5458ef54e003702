"""The anisotropic and the invariant splat variance (DSS/core/rasterizer.py:257-342) on the CPU.

  * A float64 restatement of the two modes (tests/vrk_util.py) reproduces the float64 fixtures tests/golden/vrk_*.npz -- the
    reference's own _get_per_point_info -- to 1e-10 relative, the padded-mean quirk of the invariant mode included.  This
    pins the fixtures and the formulas the GPU tests judge the kernels by.
  * The fixtures keep the share of rows with an ill-posed normal under the cap.
  * include/isopoints.h declares the four new entries and the built library exports them."""
import os
import re

import pytest
import torch

import vrk_util as VU
from conftest import ROOT

NEW_SYMBOLS = ("iso_splat_setup_vrk", "iso_splat_setup_aniso", "iso_splat_vrk_h_global", "iso_splat_vrk_h_global_work_bytes",
               "iso_splat_tangent_frame")


@pytest.mark.parametrize("scene", VU.SCENES)
def test_anisotropic_restatement_reproduces_the_fixture(scene):
    g = VU.load(scene)
    info, curv = VU.restate_aniso(g)
    e = VU.row_err(curv, g["aniso_curvature_f64"])
    print("curvature: max rel err %.3g" % e.max())
    assert e.max().item() < 1e-10
    for k in VU.KEYS:
        e = VU.row_err(info[k], g["aniso_%s_f64" % k])
        print("%s %s: max rel err %.3g" % (scene, k, e.max()))
        assert e.max().item() < 1e-10, (k, e.max().item())


@pytest.mark.parametrize("scene", VU.SCENES)
def test_invariant_restatement_reproduces_the_fixture(scene):
    g = VU.load(scene)
    h = VU.restate_invariant_h(g)
    e = ((h - g["invariant_h_f64"]).abs() / g["invariant_h_f64"]).max().item()
    print("%s h: %s, max rel err %.3g" % (scene, sorted(set(h.tolist())), e))
    assert e < 1e-10
    info = VU.restate_invariant(g, h)
    for k in VU.KEYS:
        e = VU.row_err(info[k], g["invariant_%s_f64" % k])
        print("%s %s: max rel err %.3g" % (scene, k, e.max()))
        assert e.max().item() < 1e-10, (k, e.max().item())


def test_the_fixtures_pin_the_padded_mean():
    """The sphere scene is ragged: every view cloud but the largest gets the -0.5 rows of the padding, and its h ends at the
    lower clamp although its own mean bandwidth is above the upper one; the cube's largest cloud lies between the clamps."""
    g = VU.load("sphere")
    num = g["num"].tolist()
    assert len(set(num)) == len(num)
    hs = [g["invariant_h_f64"][at].item() for at, n in VU.view_slices(g["num"])]
    for n, h in zip(num, hs):
        assert h == (1e-3 if n == max(num) else 5e-5), (num, hs)
    c = VU.load("cube")
    hc = [c["invariant_h_f64"][at].item() for at, n in VU.view_slices(c["num"])]
    assert any(5e-5 < h < 1e-3 for h in hc), hc


@pytest.mark.parametrize("scene", VU.SCENES)
def test_ill_posed_rows_stay_under_the_cap(scene):
    g = VU.load(scene)
    keep = VU.well_posed_rows(g)
    print("%s: %d of %d rows left out" % (scene, int((~keep).sum()), keep.numel()))
    assert torch.isfinite(g["aniso_radii_f64"]).all()


def test_header_declares_and_library_exports_the_new_entries():
    header = open(os.path.join(ROOT, "include", "isopoints.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
    from iso_points_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.iso_splat_vrk_h_global_work_bytes(3) > 0
