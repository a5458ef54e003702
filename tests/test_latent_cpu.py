"""Latent-conditioned SIREN (the reference's Siren(c_dim = C > 0)) on the CPU: the module reproduces the reference's
forward value and gradient from the reference's own state dict (tests/golden/make_golden_latent.py), the coded models are
recognised in both layouts while siren_spec() keeps refusing them, and the code shapes the reference's callers pass are
normalised into (codes, code_of) -- the rejected ones go to the generic route."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def load(name):
    d = np.load(os.path.join(GOLDEN, name))
    return {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}


def ours_from_golden(g):
    from iso_points_amd.sdf_models import Siren
    m = Siren(dim=3, hidden_size=int(g["hidden"]), n_layers=int(g["n_layers"]), c_dim=int(g["c_dim"]))
    m.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")})
    return m


@pytest.mark.parametrize("name", ["siren_latent_256x3.npz", "siren_latent_128x2.npz"])
def test_coded_siren_loads_the_reference_state_dict_and_reproduces_it(name):
    g = load(name)
    m = ours_from_golden(g)
    assert m.net[0].linear.in_features == 3 + int(g["c_dim"])
    c_pt = g["codes"][g["cloud"]]                                            # (P, C): every point's code
    x = g["points"].clone().requires_grad_(True)
    f = m(x, c=c_pt).sdf
    (gr,) = torch.autograd.grad([f], [x], torch.ones_like(f))
    ref_f, ref_g = g["sdf"].reshape(f.shape), g["grad"]
    assert ((f.detach() - ref_f).abs().max() / ref_f.abs().max()).item() < 1e-6
    assert ((gr - ref_g).abs().max() / ref_g.abs().max()).item() < 1e-6
    # (the float64 gradient of the golden is the same function)
    assert ((gr.double() - g["grad64"]).abs().max() / g["grad64"].abs().max()).item() < 1e-5
    # the reference's assert: code and coordinates of the same rank
    with pytest.raises(AssertionError):
        m(x.detach(), c=g["codes"][0])
    # no code: the layer-0 product fails on the width, as the reference's does
    with pytest.raises(RuntimeError):
        m(x.detach())


class _RefLayout(nn.Module):
    """The attribute layout of the reference's Siren (DSS/models/common.py:90-165): .c_dim, .net = Sequential of modules
    with .linear / .omega_0, then the linear head."""

    class _Sine(nn.Module):
        def __init__(self, i, o, w):
            super().__init__()
            self.linear, self.omega_0 = nn.Linear(i, o), w

        def forward(self, x):
            return torch.sin(self.omega_0 * self.linear(x))

    def __init__(self, c_dim, H=64, L=2):
        super().__init__()
        self.dim, self.c_dim = 3, c_dim
        self.net = nn.Sequential(self._Sine(3 + c_dim, H, 30.0), *[self._Sine(H, H, 30.0) for _ in range(L)],
                                 nn.Linear(H, 1))


def test_coded_models_are_recognised_and_siren_spec_refuses_them():
    from iso_points_amd.sdf_models import Siren, coded_siren_spec, siren_spec
    for m, C in ((Siren(hidden_size=96, n_layers=2, c_dim=32), 32), (_RefLayout(8), 8)):
        spec = coded_siren_spec(m)
        assert spec is not None and spec[3] == C and spec[1] == 30.0 and spec[2] == 30.0
        assert spec[0][0] is m.net[0].linear and len(spec[0]) == len(m.net)
        assert siren_spec(m) is None
    # unconditioned models: the other way round
    for m in (Siren(hidden_size=64, n_layers=1), _RefLayout(0)):
        assert coded_siren_spec(m) is None and siren_spec(m) is not None
    # a layer 0 whose width does not match c_dim, a sine head, too wide a network: neither
    bad = _RefLayout(8)
    bad.c_dim = 7
    assert coded_siren_spec(bad) is None
    wide = Siren(hidden_size=320, n_layers=1, c_dim=4)
    assert coded_siren_spec(wide) is None


def test_code_shapes_normalise_to_codes_and_rows():
    from iso_points_amd.sdf_models import code_rows
    C = 5
    counts = [3, 0, 2]
    base = torch.arange(3 * C, dtype=torch.float32).view(3, C)
    # one code for every point
    for c in (base[1], base[1:2], base[1:2].view(1, 1, C)):
        r = code_rows(c, C, counts)
        assert r is not None and r.code_of is None and torch.equal(r.codes, base[1:2])
    # one code per row (cloud, batch row of rays / pairs)
    for c in (base, base.view(3, 1, C), base.double()):
        r = code_rows(c, C, counts)
        assert r is not None and torch.equal(r.codes, base)
        assert r.code_of.dtype == torch.int32 and r.code_of.tolist() == [0, 0, 0, 2, 2]
    # rejected: per-point codes, a row count that is not the batch's, a broadcast middle axis, a wrong width, empty
    for c in (torch.zeros(5, C), torch.zeros(2, C), torch.zeros(3, 4, C), torch.zeros(3, C + 1), torch.zeros(0, C),
              torch.zeros(3, C, dtype=torch.int64)):
        assert code_rows(c, C, counts) is None, tuple(c.shape)


def test_fused_code_route_selection_needs_no_gpu():
    """levelset_sampling._fused_code: which calls take the fused coded route (CodeRows), which the generic one (None),
    and a coded model without its code raises, as the reference's forward does."""
    from iso_points_amd.levelset_sampling import _fused_code, _leading_rows
    from iso_points_amd.sdf_models import Siren
    m = Siren(hidden_size=64, n_layers=1, c_dim=6)
    plain = Siren(hidden_size=64, n_layers=1)
    c = torch.randn(2, 6)
    assert _fused_code(m, {"c": c}, [4, 5]) is not None
    assert _fused_code(m, {"c": c, "other": 1}, [4, 5]) is None                    # other forward kwargs: generic
    assert _fused_code(m, {"c": torch.randn(9, 6)}, [4, 5]) is None                # per-point codes: generic
    assert _fused_code(plain, {"c": c}, [4, 5]) is None                            # not a coded SIREN
    with pytest.raises(ValueError):
        _fused_code(m, {}, [9])
    assert _leading_rows((2, 7, 3)) == (2, 7) and _leading_rows((7, 3)) == (1, 7) and _leading_rows((2, 3, 4, 3)) == (2, 12)
