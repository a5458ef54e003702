"""The backward pass of the local-frame estimator (iso_pca_frames_backward) on the CPU: its oracle, and what needs no GPU.

  * the closed-form adjoint of tests/pca_backward_oracle.py equals torch autograd through torch.linalg.eigh (float64, 1e-9)
    on a noisy sphere and a cube surface, with and without the sign rule, and central differences on a small sphere (1e-6);
  * the package's rules where the formula is undefined: two equal eigenvalues, K exact duplicates;
  * the reference's NormalLoss with its autograd gradients (tests/golden/normal_loss_K16.npz) is reproduced to 1e-9;
  * the workspace helper needs no GPU; NormalLoss refuses CPU tensors and missing normals."""
import os

import numpy as np
import pytest
import torch

import pca_backward_oracle as O
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "normal_loss_K16.npz")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("cloud,P", [("sphere", 700), ("cube", 3000)])
@pytest.mark.parametrize("dis", [False, True])
def test_closed_form_equals_autograd_through_eigh(cloud, P, dis):
    K = 12
    x = (O.noisy_sphere(P, 0.05, 11) if cloud == "sphere" else O.cube_surface(P, 0.01, 12)).double()
    idx = O.brute_knn(x, K)
    w, F = O.frames_fixed(x, idx, None, dis)
    # rows whose gaps are all >= 1e-2 l_max carry gradients; the others get none (torch's eigh backward is unbounded there)
    g_l, g_V, _ = O.incoming(P, 3, w.numpy(), (0, 1, 2))
    sep = torch.from_numpy(O.min_gap(w.numpy(), (0, 1, 2)) >= O.WELL_SEPARATED)
    g_l = g_l * sep[:, None]
    assert sep.double().mean() > 0.5, "too few well-separated rows to mean anything"
    want = O.autograd_grad(x, idx, F, dis, g_l, g_V)
    got, _, _ = O.closed_form(x, idx, F, dis, g_l, g_V)
    print("%s dis=%s: %d of %d rows well separated, closed form vs autograd %.3e" % (cloud, dis, int(sep.sum()), P,
                                                                                    _rel(got, want)))
    assert _rel(got, want) <= 1e-9


@pytest.mark.parametrize("dis", [False, True])
def test_closed_form_equals_central_differences(dis):
    P, K = 64, 8
    x = O.noisy_sphere(P, 0.05, 21).double()
    idx = O.brute_knn(x, K)
    w, F = O.frames_fixed(x, idx, None, dis)
    F = F.detach()
    g_l, g_V, _ = O.incoming(P, 4, w.numpy(), (0, 1, 2))
    got, _, _ = O.closed_form(x, idx, F, dis, g_l, g_V)

    def loss(xx):
        ww, FF = O.frames_fixed(xx, idx, F, dis)           # index and signs held fixed
        return float((ww * g_l).sum() + (FF * g_V).sum())
    h = 1e-6
    fd = torch.zeros_like(x)
    for i in range(P):
        for c in range(3):
            xp, xm = x.clone(), x.clone()
            xp[i, c] += h
            xm[i, c] -= h
            fd[i, c] = (loss(xp) - loss(xm)) / (2 * h)
    print("dis=%s: closed form vs central differences %.3e" % (dis, _rel(got, fd)))
    assert _rel(got, fd) <= 1e-6


def test_rules_where_the_formula_is_undefined():
    # row 0: C = diag(1/3, 1/3, 3) exactly -- two equal eigenvalues; row 1: K exact duplicates
    sq = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 3.0], [0, 0, -3.0]], dtype=torch.float64)
    x = torch.cat([sq, torch.full((6, 3), 0.5, dtype=torch.float64)])
    idx = torch.stack([torch.arange(6), torch.arange(6, 12)])
    g = torch.Generator().manual_seed(0)
    g_l = torch.randn(2, 3, generator=g, dtype=torch.float64)
    g_V = torch.randn(2, 3, 3, generator=g, dtype=torch.float64)
    for dis in (False, True):
        for dtype in (torch.float64, torch.float32):
            grad, w, _ = O.closed_form(x, idx, None, dis, g_l, g_V, dtype=dtype)
            assert torch.isfinite(grad).all()
            assert abs(float(w[0, 0] - w[0, 1])) <= O.GAP_RULE * float(w[0, 2]), "the test's row has no equal pair"
            assert float(w[1].max()) == 0.0 and (grad[6:] == 0).all(), "K duplicates: l_max = 0 gives a zero gradient"
    # the equal pair exchanges nothing: incoming gradients that only turn v_0 and v_1 within their own plane (g_0 = v_1,
    # g_1 = -v_0) have S_01 as their one term in the plain formula, and the rule takes it out
    _, F = O.frames_fixed(x, idx)
    g_rot = torch.zeros(2, 3, 3, dtype=torch.float64)
    g_rot[0, :, 0], g_rot[0, :, 1] = F[0, :, 1], -F[0, :, 0]
    grad, _, _ = O.closed_form(x, idx, F, False, torch.zeros(2, 3, dtype=torch.float64), g_rot)
    assert float(grad.abs().max()) <= 1e-12
    # a planar neighbourhood: its smallest eigenvalue is 0 (clamped or exact) and passes no gradient
    flat = torch.cat([sq[:4], torch.tensor([[0.3, 0.3, 0.0], [-0.4, 0.1, 0.0]], dtype=torch.float64)])
    gl = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64)
    grad, w, _ = O.closed_form(flat, torch.arange(6)[None], None, False, gl, torch.zeros(1, 3, 3, dtype=torch.float64))
    assert float(w[0, 0]) <= 1e-16 and float(grad.abs().max()) <= 1e-12


def test_work_bytes_needs_no_gpu_and_grows():
    from iso_points_amd import _lib
    lib = _lib.load()
    f = lib.iso_pca_frames_backward_work_bytes
    assert f(1, 1000, 8) > 0
    assert f(1, 2000, 8) > f(1, 1000, 8)
    assert f(1, 1000, 16) > f(1, 1000, 8)
    assert f(2, 1000, 8) > f(1, 1000, 8)
    # at least the adjoint (9 floats per row), the slots' targets and the lists (3 ints per slot)
    assert f(1, 1000, 8) >= 4 * (9 * 1000 + 3 * 8 * 1000)
    assert f(0, 1000, 8) >= 0


def test_normal_loss_refuses_cpu_tensors_and_missing_normals():
    from iso_points_amd.loss import NormalLoss, ProjectionLoss, RepulsionLoss   # exported beside the other two
    assert ProjectionLoss and RepulsionLoss
    x = torch.nn.functional.normalize(torch.randn(1, 200, 3, generator=torch.Generator().manual_seed(0)), dim=-1)
    loss = NormalLoss(neighborhood_size=8)
    assert loss.reduction == "mean" and NormalLoss().neighborhood_size == 16
    with pytest.raises(RuntimeError, match="GPU"):
        loss((x, x.clone()))
    with pytest.raises(ValueError):
        loss(x)                                             # a bare tensor has no normals

    class NoNormals(object):
        def points_padded(self):
            return x

        def num_points_per_cloud(self):
            return torch.tensor([200])

        def normals_padded(self):
            return None
    with pytest.raises(ValueError):
        loss(NoNormals())
    with pytest.raises(ValueError):
        NormalLoss(reduction="median")
    with pytest.raises(ValueError):
        loss((x, x.clone()), reduction="median")


def test_oracle_reproduces_the_reference_normal_loss():
    d = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert set(d.files) == {"points", "normals", "idx", "K", "loss", "grad_points", "grad_normals"}
    for k in d.files:
        assert d[k].dtype.kind in "fiu", k                  # arrays only
    x = torch.from_numpy(d["points"][0]).double().requires_grad_(True)
    n = torch.from_numpy(d["normals"][0]).double().requires_grad_(True)
    idx = torch.from_numpy(d["idx"][0]).long()
    assert idx.shape == (1500, 16) and int(d["K"]) == 16
    loss = O.normal_loss(x, n, idx)
    g_x, g_n = torch.autograd.grad(loss.sum(), (x, n))
    for got, want, what in ((loss.detach(), d["loss"], "loss"), (g_x, d["grad_points"][0], "grad_points"),
                            (g_n, d["grad_normals"][0], "grad_normals")):
        e = _rel(got, torch.from_numpy(np.asarray(want)))
        print("%s: oracle vs the reference %.3e" % (what, e))
        assert e <= 1e-9, what
    # the closed form gives the same point gradient from the loss's gradient w.r.t. the PCA normal
    _, F = O.frames_fixed(x.detach(), idx)
    nr = F[:, :, 0].clone().requires_grad_(True)
    (g_nr,) = torch.autograd.grad((1 - torch.nn.functional.cosine_similarity(n.detach(), nr).abs()).sum(), nr)
    g_V = torch.zeros(1500, 3, 3, dtype=torch.float64)
    g_V[:, :, 0] = g_nr
    got, _, _ = O.closed_form(x, idx, F, False, torch.zeros(1500, 3, dtype=torch.float64), g_V)
    assert _rel(got, torch.from_numpy(d["grad_points"][0])) <= 1e-9
