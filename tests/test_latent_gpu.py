"""Latent-conditioned SIREN (the reference's Siren(c_dim = C > 0)) on the fused kernels.

The code only moves layer 0's bias (b_u = b0 + W0[:, :C] c_u), so the kernels take a per-code bias table
(iso_siren_fold_codes) and otherwise run the network of the xyz columns.  What is pinned here:
  * the fold against float64;
  * bit-identity: a coded evaluation with code u equals the uncoded evaluation of the network whose b0 is table row u
    (projection, value + gradient, sphere tracing; one code, and one code per ragged cloud in one call);
  * parity with the reference's own Siren(c_dim = 32) (tests/golden/make_golden_latent.py), judged as
    tests/test_golden_gpu.py judges the unconditioned SIREN goldens;
  * the reference's call shapes take the fused route (no generic-route warning) and agree with float64;
  * a full-size repeat-stress of the coded split-fp16 kernels (the instantiations under the spill allow-list keys)."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")


def load(name):
    d = np.load(os.path.join(GOLDEN, name))
    return {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}


def coded_siren(H, L, C, seed):
    from iso_points_amd.sdf_models import Siren
    torch.manual_seed(seed)
    return Siren(hidden_size=H, n_layers=L, c_dim=C)


def folded(m, bias_row):
    """The unconditioned network of m's xyz columns whose layer-0 bias is `bias_row` (a table row, first H entries)."""
    from iso_points_amd.sdf_models import Siren
    C = m.c_dim
    H = m.net[0].linear.out_features
    f = Siren(hidden_size=H, n_layers=len(m.net) - 2, c_dim=0).to(m.net[0].linear.weight.device)
    with torch.no_grad():
        f.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("net.0.")}, strict=False)
        f.net[0].linear.weight.copy_(m.net[0].linear.weight[:, C:])
        f.net[0].linear.bias.copy_(bias_row[:H])
    return f


def table_of(m, codes):
    from iso_points_amd.sdf_models import PackedSiren
    t = PackedSiren(m, codes.device).fold(codes)
    torch.cuda.synchronize()
    return t


def cloud(P, seed, scale=1.6):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) - 0.5) * scale


# ---------------------------------------------------------------------------------------------------- 1. the fold
@pytest.mark.parametrize("C", [1, 32, 256])
@pytest.mark.parametrize("H", [128, 256, 96])
def test_fold_matches_float64(dev, C, H):
    m = coded_siren(H, 1, C, seed=C + H).to(dev)
    codes = torch.randn(5, C, device=dev)
    t = table_of(m, codes)
    Hp = next(h for h in (64, 128, 256) if h >= H)
    assert t.shape == (5, Hp)
    W = m.net[0].linear.weight.detach().double()[:, :C]
    b = m.net[0].linear.bias.detach().double()
    want = b[None, :] + codes.double() @ W.t()
    bound = 2.0 ** -22 * (b.abs()[None, :] + codes.double().abs() @ W.abs().t())
    err = (t[:, :H].double() - want).abs()
    assert (err <= bound).all(), (err / bound).max().item()
    assert (t[:, H:] == 0).all()


# ------------------------------------------------------------------------------------ 2. bit-identity, one code
@pytest.mark.parametrize("H,L", [(256, 3), (128, 2), (64, 2)])
def test_one_code_is_bit_identical_to_the_folded_network(dev, gemm_mode, H, L):
    from iso_points_amd.levelset_sampling import SphereTracing, UniformProjection, full_lengths
    C = 32
    m = coded_siren(H, L, C, seed=H + L).to(dev)
    code = torch.randn(C, device=dev)
    f = folded(m, table_of(m, code.view(1, C))[0])
    x = cloud(4000, seed=H).to(dev).unsqueeze(0)
    for T in (1, 10):
        up = UniformProjection(proj_tolerance=1e-30)
        a = up._project_points(m, x, full_lengths(x), proj_max_iters=T, c=code)
        b = UniformProjection(proj_tolerance=1e-30)._project_points(f, x, full_lengths(x), proj_max_iters=T)
        for u, v in zip(a, b):
            assert torch.equal(u, v), T
        assert not torch.equal(a.points, x)
    up = UniformProjection()
    for c in (code, code.view(1, C)):
        s1, g1 = up._compute_sdf_and_grad(x, m, c=c)
        s2, g2 = up._compute_sdf_and_grad(x, f)
        assert torch.equal(s1, s2) and torch.equal(g1, g2)
    # sphere tracing from a sphere of radius 0.9 towards the centre
    d = -torch.nn.functional.normalize(x, dim=-1)
    r0 = -0.9 * d
    st = SphereTracing(proj_max_iters=10)
    a = st.project_points(r0, d, m, latent=code.view(1, C))
    b = st.project_points(r0, d, f)
    for k in ("levelset_points", "network_eval_on_levelset_points", "mask"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------ 3. bit-identity, a code per cloud
@pytest.mark.parametrize("H,L", [(256, 3), (128, 2)])
def test_code_per_cloud_is_bit_identical_cloud_by_cloud(dev, gemm_mode, H, L):
    from iso_points_amd.levelset_sampling import UniformProjection, _ClipLengths, full_lengths
    C = 32
    m = coded_siren(H, L, C, seed=7 * H + L).to(dev)
    codes = torch.randn(3, C, device=dev)
    table = table_of(m, codes)
    sizes = [3000, 1234, 2077]
    clouds = [cloud(n, seed=11 + i).to(dev) for i, n in enumerate(sizes)]
    padded = torch.zeros(3, max(sizes), 3, device=dev)
    for i, p in enumerate(clouds):
        padded[i, :sizes[i]] = p
    lengths = torch.tensor(sizes, device=dev)
    out = UniformProjection().project_points(_ClipLengths(padded, lengths), m, skip_resampling=True,
                                             skip_upsampling=True, c=codes)
    for i, p in enumerate(clouds):
        x = p.unsqueeze(0)
        want = UniformProjection()._project_points(folded(m, table[i]), x, full_lengths(x), proj_max_iters=10)
        n = sizes[i]
        assert torch.equal(out["levelset_points"][i, :n], want.points[0])
        assert torch.equal(out["mask"][i, :n], want.mask[0])
        if "levelset_normals" in out:           # (absent when no point converged: the reference's early return, :396)
            assert torch.equal(out["levelset_normals"][i, :n], want.normals[0])


# ---------------------------------------------------------------------------------- 4. parity with the reference
@pytest.mark.parametrize("name", ["siren_latent_256x3.npz", "siren_latent_128x2.npz"])
def test_coded_siren_vs_the_reference_siren_class(dev, gemm_mode, name):
    """Value and gradient at 1e-5 relative, and 4 Newton moves judged against the float64 iteration of the same model
    (oracle/iso_oracle.py with a per-point code, one chunk) quantile by quantile, as the reference's own float32 run
    deviates from it, plus agreement with the golden on the bulk of the points."""
    from oracle import iso_oracle as O
    from iso_points_amd.levelset_sampling import UniformProjection
    from iso_points_amd.sdf_models import CodeRows, Siren, siren_sdf_and_grad
    from util import rel_err
    g = load(name)
    m = Siren(dim=3, hidden_size=int(g["hidden"]), n_layers=int(g["n_layers"]), c_dim=int(g["c_dim"]))
    m.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd/")})
    m64 = copy.deepcopy(m).double()
    m = m.to(dev)
    codes, cl, x = g["codes"], g["cloud"], g["points"]
    sdf, grad = siren_sdf_and_grad(m, x.to(dev), code=CodeRows(codes.to(dev), cl.to(torch.int32).to(dev)))
    assert rel_err(sdf, g["sdf"]) < 1e-5 and rel_err(grad, g["grad"]) < 1e-5
    assert rel_err(sdf, g["sdf64"]) < 1e-5 and rel_err(grad, g["grad64"]) < 1e-5
    # 4 Newton moves, one code per cloud (the golden's points are the three clouds in order)
    sizes = [int((cl == i).sum()) for i in range(codes.shape[0])]
    padded = torch.zeros(len(sizes), max(sizes), 3)
    s = 0
    for i, n in enumerate(sizes):
        padded[i, :n] = x[s:s + n]
        s += n
    T = int(g["T"])
    r = UniformProjection(proj_tolerance=1e-30)._project_points(m, padded.to(dev), torch.tensor(sizes, device=dev),
                                                                proj_max_iters=T, c=codes.to(dev))
    ours = torch.cat([r.points[i, :n].cpu() for i, n in enumerate(sizes)])
    r64 = O.project_points(m64, x.double().unsqueeze(0), torch.tensor([x.shape[0]]), proj_max_iters=T,
                           proj_tolerance=1e-30, max_points_per_pass=x.shape[0], c=codes.double()[cl])
    p64 = r64.points[0]
    scale = p64.abs().max()
    e_ref = ((g["fixed_points"].double() - p64).abs().amax(-1) / scale).view(-1)
    e_our = ((ours.double() - p64).abs().amax(-1) / scale).view(-1)
    # (the single worst point of a random, chaotic network gets a wider factor: measured 3.1 on the f32-MFMA 128 x 2 case,
    # whose uncoded kernel computes the same bits -- test_one_code_is_bit_identical_to_the_folded_network)
    for q, k in ((0.5, 1.5), (0.9, 1.5), (0.99, 1.5), (1.0, 5.0)):
        assert torch.quantile(e_our, q) <= k * torch.quantile(e_ref, q) + 2e-7, \
            (q, torch.quantile(e_our, q).item(), torch.quantile(e_ref, q).item())
    e_g = ((ours - g["fixed_points"]).abs().amax(-1) / g["fixed_points"].abs().max()).view(-1)
    assert (e_g > 1e-5).float().mean() < 0.006 and e_g.median() < 1e-6


# ------------------------------------------------------------------------- 5. the reference's call shapes, no warning
class _WithCode(torch.nn.Module):
    """model.forward(x) = m(x, c = code for every row of x): the reference's forward with one code, for a loop that
    compacts its points between evaluations"""

    def __init__(self, m, code):
        super().__init__()
        self.m, self.code = m, code

    def forward(self, x, **kw):
        return self.m(x, c=self.code.expand(x.shape[0], -1))


def test_reference_call_shapes_take_the_fused_route(dev):
    from oracle import iso_oracle as O
    from iso_points_amd.levelset_sampling import (SphereTracing, UniformProjection, _ClipLengths,
                                                  find_zero_crossing_between_point_pairs)
    C, N = 32, 2
    m = coded_siren(128, 2, C, seed=5)
    m64 = copy.deepcopy(m).double()
    m = m.to(dev)
    c = torch.randn(N, C, device=dev)

    def f64(pts, rows):                                  # float64 value of the reference-shaped model, code of each row
        with torch.no_grad():
            return m64(pts.detach().cpu().double().reshape(-1, 3), c=c.cpu().double()[rows]).sdf.reshape(-1)

    P = 2500
    pts = torch.stack([cloud(P, seed=40 + i) for i in range(N)]).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        # combined_modeling.py:449 / implicit_modeling.py:156-159 (projection of N clouds, one code each)
        out = UniformProjection().project_points(_ClipLengths(pts, torch.tensor([P] * N, device=dev)), m,
                                                 skip_resampling=True, skip_upsampling=True, c=c)
        # implicit_modeling.py:305,313: rays (N, R, 3), latent (N, C)
        R = P
        d = -torch.nn.functional.normalize(pts, dim=-1)
        tr = SphereTracing().project_points(-0.9 * d, d, m, latent=c)
        # implicit_modeling.py:318-319: pairs (N, R, 3), c (N, C)
        p0, p1 = -0.9 * d, 0.9 * d
        zc, zmask = find_zero_crossing_between_point_pairs(p0, p1, m, c=c, is_occupancy=False)
    for i in range(N):       # the float64 loop of the reference, cloud by cloud with that cloud's code
        ref = O.project_points(_WithCode(m64, c[i].cpu().double()), pts[i:i + 1].cpu().double(), torch.tensor([P]),
                               proj_max_iters=10)
        # a random network is not an SDF: judged on the bulk, as the goldens are (a few chaotic points drift apart)
        e = ((out["levelset_points"][i].cpu().double() - ref.points[0]).abs().amax(-1) / ref.points.abs().max())
        assert (e > 1e-5).float().mean() < 0.01 and e.median() < 1e-6, ((e > 1e-5).sum().item(), e.median().item())
    rows_r = torch.arange(N).repeat_interleave(R)
    val = tr["network_eval_on_levelset_points"].reshape(-1).cpu().double()
    want = f64(tr["levelset_points"], rows_r)
    assert ((val - want).abs().max() / want.abs().max()).item() < 1e-5
    assert tr["mask"].any()
    # the secant's roots are roots of the float64 model (values are O(0.1) on this network)
    zm = zmask.reshape(-1).cpu()
    assert zm.sum() > 100
    assert f64(zc, rows_r)[zm].abs().max().item() < 1e-3


# -------------------------------------------------------------------------------------- 6. full-size repeat-stress
def test_coded_siren_repeat_stress_1m(dev):
    """1 M points, 256 x 3, three codes, T = 10, ten repeats: every repeat bit-identical (the coded split-fp16 kernels
    that fall under the spill allow-list keys of tests/test_abi.py, k_siren_step_x3_both<256, 8, 3, 1, CODED> and the
    Newton tail)."""
    from iso_points_amd import _lib
    from iso_points_amd.levelset_sampling import UniformProjection
    assert _lib.load().iso_siren_get_gemm_mode() == 1
    m = coded_siren(256, 3, 32, seed=3).to(dev)
    codes = torch.randn(3, 32, device=dev)
    sizes = [400_000, 350_000, 250_000]
    pts = torch.zeros(3, max(sizes), 3, device=dev)
    for i, n in enumerate(sizes):
        pts[i, :n] = cloud(n, seed=90 + i).to(dev)
    lengths = torch.tensor(sizes, device=dev)
    up = UniformProjection()
    first = up._project_points(m, pts, lengths, proj_max_iters=10, c=codes)
    for _ in range(10):
        r = up._project_points(m, pts, lengths, proj_max_iters=10, c=codes)
        for u, v in zip(r, first):
            assert torch.equal(u, v)
