"""The IDR SDF's backward (csrc/idrgrad.hip, iso_idrgrad_backward; sdf_models._IdrFunction / idr_forward / sdf_forward /
get_normals_from_grad) against torch's double backward of the same network in float64 on the CPU.  Oracle and criterion:
tests/idr_backward_oracle.py (the rule of tests/siren_backward_oracle.py: e_hip <= 1.5 max(e_cpu32, e_gpu32) + 2e-7 per
gradient tensor, no point filtered, every figure printed before anything is asserted).

The kernels are called directly (abi_grads: NaN-guarded inputs, NaN-filled outputs and workspace) where the effective
weights' gradients are looked at, and through idr_forward and torch's backward where the parameters' are."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from idr_backward_oracle import (BETA, abi_grads, assert_criterion, make_net, make_points, raw_of, references, seeded_UV,
                                 shape_of)
from siren_backward_oracle import FACTOR, FLOOR, err, nan_like

pytestmark = pytest.mark.gpu

N = 800
FORMS = [(128, 2, None, 0), (128, 3, 1, 4), (256, 4, 2, 6), (256, 4, 3, 10), (512, 2, None, 6), (512, 8, 4, 6), (128, 12, 6, 6)]
VALUE_ONLY = [(128, 3, 1, 4), (256, 4, 2, 6), (512, 2, None, 6)]
SMALL = (128, 2, None, 0)            # the smallest shape: the point counts and the two workspace chunks
SKIPPED = (128, 3, 1, 4)


def _id(shape):
    return "H%d_n%d_skip%s_F%d" % shape


def run(shape, n, dev, seed, U=None, V="seeded", scale=1.0, what=None):
    net = make_net(*shape, seed=seed)
    pts = make_points(n, seed=seed + 1, scale=scale)
    sU, sV = seeded_UV(n, seed)
    U = sU if U is None else U
    V = sV if isinstance(V, str) else V
    refs = references(net, pts, U, V, dev)
    got = abi_grads(net, pts, U, V, dev)
    assert_criterion(got, refs, what or (shape, n), shape[1])
    return net, pts, U, V, got, refs


@pytest.mark.parametrize("shape", FORMS, ids=_id)
def test_forms_and_depths(dev, shape):
    run(shape, N, dev, seed=shape[0] + shape[1])


@pytest.mark.parametrize("shape", VALUE_ONLY, ids=_id)
def test_value_only_is_the_first_order_backward(dev, shape):
    """v absent: the gradient of sum(U f) alone, on the form without tangent columns"""
    net, pts, U, V, got, refs = run(shape, N, dev, seed=21 + shape[1], V=None)
    # ... and the tangent form run on v = 0 gives the same mathematics
    zero = abi_grads(net, pts, U, torch.zeros(N, 3), dev)
    assert_criterion(zero, refs, (shape, "v = 0"), shape[1])


def test_point_counts_around_the_tile_and_the_partial_chunk(dev):
    from iso_points_amd import _lib
    chunk = _lib.load().iso_idrgrad_chunk_points()
    assert chunk >= 66
    for n in (1, 7, 8, 9, 31, 32, 33, chunk - 1, chunk, chunk + 1):      # a tile is 32 points with tangent columns
        run(SKIPPED, n, dev, seed=n)
    for n in (1, 63, 64, 65, chunk + 1):                                  # ... and 64 without
        run(SKIPPED, n, dev, seed=n, V=None)


def test_two_workspace_chunks_and_slices(dev):
    """More points than one workspace chunk holds: the weight gradients against float64 (the second chunk adds onto the
    first), and the same points run alone give the same bits in their rows of d points."""
    from iso_points_amd import _lib
    wsp = _lib.load().iso_idrgrad_workspace_points()
    n = wsp + 37
    net, pts, U, V, full, _ = run(SMALL, n, dev, seed=11)
    for lo, hi in ((0, 1), (0, 33), (100, 230), (wsp - 5, wsp), (wsp, n), (wsp - 40, wsp + 9)):
        got = abi_grads(net, pts[lo:hi].contiguous(), U[lo:hi].contiguous(), V[lo:hi].contiguous(), dev, want_raw=False)
        assert torch.equal(got["points"], full["points"][lo:hi]), (lo, hi)


def test_gradient_only(dev):
    run((256, 4, 2, 6), N, dev, seed=31, U=torch.zeros(N))


def test_one_live_point(dev):
    n, live = 700, 333
    U, V = torch.zeros(n), torch.zeros(n, 3)
    sU, sV = seeded_UV(n, 41)
    U[live], V[live] = sU[live], sV[live]
    net, pts, U, V, got, refs = run(SKIPPED, n, dev, seed=41, U=U, V=V)
    dead = torch.ones(n, dtype=torch.bool)
    dead[live] = False
    assert (got["points"][dead] == 0).all() and got["points"][live].abs().max() > 0


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_scaled_points(dev, scale):
    """the arguments of the encoding's sines: tiny, and (at 2^5 x 3) many periods"""
    run((256, 4, 2, 6), N, dev, seed=51, scale=scale)


def test_two_calls_give_the_same_bits(dev):
    net = make_net(*SKIPPED, seed=61)
    n = 2 * 256 + 77
    pts = make_points(n, seed=62)
    U, V = seeded_UV(n, 61)
    a, b = abi_grads(net, pts, U, V, dev), abi_grads(net, pts, U, V, dev)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _abi_setup(net, n, dev, seed):
    from iso_points_amd import _lib
    lib = _lib.load()
    H, nl, skip, nf = shape_of(net)
    raw = raw_of(net).to(dev)
    packed = torch.empty((lib.iso_idr_packed_floats(H, nl) + 4,), dtype=torch.float32, device=dev)
    _lib.call("iso_idr_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, nl, skip, nf, _lib.stream())
    pts = make_points(n, seed=seed).to(dev)
    U, V = (t.to(dev) for t in seeded_UV(n, seed))
    need = lib.iso_idrgrad_workspace_bytes(n, H, nl, skip, nf)
    ws = nan_like((need // 4 + 4,), dev)
    return lib, raw, packed, pts, U, V, need, ws


def test_null_outputs_select_the_work(dev):
    """grad_raw_out NULL: d points alone, the same bits; grad_pts_out NULL: the weight gradients alone, the same bits; both
    NULL: nothing is launched and the workspace stays as it was"""
    from iso_points_amd import _lib
    net = make_net(*SKIPPED, seed=71)
    n = 300
    pts = make_points(n, seed=72)
    U, V = seeded_UV(n, 71)
    full = abi_grads(net, pts, U, V, dev)
    only_p = abi_grads(net, pts, U, V, dev, want_raw=False)
    only_w = abi_grads(net, pts, U, V, dev, want_pts=False)
    assert sorted(only_p) == ["points"] and "points" not in only_w
    assert torch.equal(only_p["points"], full["points"])
    for k in only_w:
        assert torch.equal(only_w[k], full[k]), k
    lib, raw, packed, d_pts, d_u, d_v, need, ws = _abi_setup(net, n, dev, 72)
    H, nl, skip, nf = shape_of(net)
    _lib.call("iso_idrgrad_backward", _lib.ptr(d_pts), _lib.ptr(d_u), _lib.ptr(d_v), n, _lib.ptr(raw), _lib.ptr(packed), H, nl,
              skip, nf, BETA, None, None, _lib.ptr(ws), need, _lib.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()


def test_refusals_launch_nothing(dev):
    from iso_points_amd import _lib
    n = 100
    net = make_net(*SKIPPED, seed=151)
    H, nl, skip, nf = shape_of(net)
    lib, raw, packed, pts, U, V, need, ws = _abi_setup(net, n, dev, 152)
    g_raw, g_pts = nan_like((raw.numel(),), dev), nan_like((n, 3), dev)
    P = _lib.ptr
    st = _lib.stream()

    def call(**kw):
        a = dict(pts=P(pts), u=P(U), v=P(V), n=n, raw=P(raw), packed=P(packed), H=H, nl=nl, skip=skip, nf=nf, beta=BETA,
                 g_raw=P(g_raw), g_pts=P(g_pts), ws=P(ws), bytes=need)
        a.update(kw)
        return lib.iso_idrgrad_backward(a["pts"], a["u"], a["v"], a["n"], a["raw"], a["packed"], a["H"], a["nl"], a["skip"],
                                        a["nf"], a["beta"], a["g_raw"], a["g_pts"], a["ws"], a["bytes"], st)
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    for H_bad in (0, 64, 127, 129, 384, 1024):
        assert call(H=H_bad) == UNSUPPORTED, H_bad
    assert call(nl=1) == UNSUPPORTED and call(nl=13) == UNSUPPORTED
    assert call(skip=0) == UNSUPPORTED and call(skip=nl) == UNSUPPORTED
    assert call(nf=11) == UNSUPPORTED and call(nf=-1) == UNSUPPORTED
    assert call(beta=50.0) == UNSUPPORTED and call(beta=100.5) == UNSUPPORTED
    assert call(n=-1) == INVALID
    for k in ("pts", "u", "packed", "ws"):
        assert call(**{k: None}) == INVALID, k
    assert call(bytes=need - 1) == WORKSPACE and call(bytes=0) == WORKSPACE
    assert call(ws=ctypes.c_void_p(ws.data_ptr() + 4)) == INVALID
    assert call(packed=ctypes.c_void_p(packed.data_ptr() + 4)) == INVALID
    assert b"iso_idrgrad_backward" in lib.iso_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(g_raw).all() and torch.isnan(g_pts).all() and torch.isnan(ws).all()
    # n = 0: nothing to sum, zeros; the points' output is not touched
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (g_raw == 0).all() and torch.isnan(g_pts).all() and torch.isnan(ws).all()
    # and the accepted call at the exact workspace size, raw NULL (it is not read)
    assert call(raw=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(g_raw).all() and torch.isfinite(g_pts).all()


# ---- through idr_forward and torch's backward -------------------------------------------------------------------------------
class RefLike(nn.Module):
    """laid out like the reference's SDF (tests/test_idr_gpu.py::test_reference_style_module_is_recognised builds the same)"""

    def __init__(self, H=128, n_layers=3, skip_in=(2,), F=4):
        super().__init__()
        d0 = 3 + 6 * F
        dims = [d0] + [H] * n_layers + [1]
        self.num_layers, self.skip_in, self.F = len(dims), skip_in, F
        self.embed_fn = lambda x: torch.cat([x] + [f(x * 2.0 ** k) for k in range(F) for f in (torch.sin, torch.cos)], -1)
        for l in range(self.num_layers - 1):
            out = dims[l + 1] - d0 if (l + 1) in skip_in else dims[l + 1]
            setattr(self, "lin%d" % l, nn.utils.weight_norm(nn.Linear(dims[l], out)))
        self.softplus = nn.Softplus(beta=100)

    def forward(self, inp, **kw):
        from oracle.iso_oracle import SdfOut
        inp = self.embed_fn(inp)
        x = inp
        for l in range(self.num_layers - 1):
            if l in self.skip_in:
                x = torch.cat([x, inp], -1) / np.sqrt(2)
            x = getattr(self, "lin%d" % l)(x)
            if l < self.num_layers - 2:
                x = self.softplus(x)
        return SdfOut(sdf=torch.tanh(x))


def _reflike(seed=82):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.random.fork_rng():
            torch.manual_seed(seed)
            return RefLike()


def module_grads(build, pts, lossfn, dtype, device, fused=False):
    """{parameter name: grad, points} as float64 CPU tensors of lossfn(f, g); fused: through idr_forward"""
    from iso_points_amd.sdf_models import idr_forward
    m = build().to(dtype).to(device)
    p = pts.to(dtype).to(device).detach().requires_grad_(True)
    if fused:
        f, g = idr_forward(m, p)
        assert f.grad_fn is not None and g.grad_fn is not None
    else:
        f = m(p).sdf.squeeze(-1)
        g = torch.autograd.grad(f.sum(), p, create_graph=True)[0]
    lossfn(f, g).backward()
    if device != "cpu":
        torch.cuda.synchronize()
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().double().cpu() for k, v in m.named_parameters()}
    out["points"] = p.grad.detach().double().cpu()
    return out


def uv_loss(U, V):
    return lambda f, g: (U.to(f) * f).sum() + (V.to(g) * g).sum()


def assert_rule(got, refs, what):
    g64, g32c, g32g = refs
    assert sorted(got) == sorted(g64), (sorted(got), sorted(g64))
    rows = []
    for k in sorted(got):
        e_hip, e_cpu, e_gpu = err(got[k], g64[k]), err(g32c[k], g64[k]), err(g32g[k], g64[k])
        print("%s %s: e_cpu %.3g e_gpu %.3g e_hip %.3g ratio %.3f" % (what, k, e_cpu, e_gpu, e_hip,
                                                                       e_hip / (FACTOR * max(e_cpu, e_gpu) + FLOOR)))
        rows.append((k, e_cpu, e_gpu, e_hip))
    for k, e_cpu, e_gpu, e_hip in rows:
        assert torch.isfinite(got[k]).all() and got[k].shape == g64[k].shape, (what, k)
        assert e_hip <= FACTOR * max(e_cpu, e_gpu) + FLOOR, (what, k, e_cpu, e_gpu, e_hip)


def module_refs(build, pts, lossfn, dev):
    return (module_grads(build, pts, lossfn, torch.float64, "cpu"), module_grads(build, pts, lossfn, torch.float32, "cpu"),
            module_grads(build, pts, lossfn, torch.float32, dev))


@pytest.mark.parametrize("which", ["oracle_module", "reference_layout"])
def test_idr_forward_trains_every_parameter(dev, which):
    """v, g, b of the oracle's IdrSDF; weight_g, weight_v, bias of a module built with nn.utils.weight_norm; the points"""
    from iso_points_amd.sdf_models import idr_spec
    build = (lambda: make_net(*SKIPPED, seed=81)) if which == "oracle_module" else _reflike
    names = [k for k, _ in build().named_parameters()]
    assert idr_spec(build()) is not None
    assert any(k.endswith("weight_g") for k in names) if which == "reference_layout" else any(k.startswith("g.") for k in names)
    pts = make_points(600, seed=83)
    lossfn = uv_loss(*seeded_UV(600, 81))
    got = module_grads(build, pts, lossfn, torch.float32, dev, fused=True)
    assert_rule(got, module_refs(build, pts, lossfn, dev), which)


def test_requires_grad_subsets(dev):
    """only the points; only the weights; only one layer's bias: what needs no gradient gets none, the rest is unchanged"""
    from iso_points_amd.sdf_models import idr_forward
    net = make_net(*SKIPPED, seed=91).to(dev)
    pts = make_points(300, seed=92).to(dev)
    U, V = (t.to(dev) for t in seeded_UV(300, 91))

    def grads(p_grad, names):
        m = copy.deepcopy(net)
        for k, v in m.named_parameters():
            v.requires_grad_(names is None or k in names)
        p = pts.clone().requires_grad_(p_grad)
        f, g = idr_forward(m, p)
        ((U * f).sum() + (V * g).sum()).backward()
        out = {k: v.grad for k, v in m.named_parameters()}
        out["points"] = p.grad
        return out
    full = grads(True, None)
    assert all(v is not None for v in full.values())
    for p_grad, names in ((True, ()), (False, None), (False, ("b.1",))):
        got = grads(p_grad, names)
        for k, v in got.items():
            wanted = p_grad if k == "points" else (names is None or k in names)
            assert (v is not None) == wanted, (p_grad, names, k)
            if wanted:
                assert torch.equal(v, full[k]), (p_grad, names, k)


def test_idr_forward_without_grad_is_the_detached_route(dev):
    from iso_points_amd.sdf_models import idr_forward, idr_sdf_and_grad
    m = make_net(*SKIPPED, seed=131).to(dev)
    p = make_points(777, seed=132).to(dev)
    f0, g0 = idr_sdf_and_grad(m, p)
    with torch.no_grad():
        f1, g1 = idr_forward(m, p)
    for v in m.parameters():
        v.requires_grad_(False)
    f2, g2 = idr_forward(m, p)
    f3, g3 = idr_forward(m, p, need_grad=False)
    assert g3 is None and f1.grad_fn is None and f2.grad_fn is None
    for f, g in ((f1, g1), (f2, g2)):
        assert torch.equal(f, f0) and torch.equal(g, g0)
    assert torch.equal(f3, idr_sdf_and_grad(m, p, need_grad=False)[0])      # the value-only kernel form has its own bits
    # ... and under grad the values are the same evaluation's
    for v in m.parameters():
        v.requires_grad_(True)
    f4, g4 = idr_forward(m, p)
    assert f4.grad_fn is not None and torch.equal(f4.detach(), f0) and torch.equal(g4.detach(), g0)


def test_get_normals_from_grad_and_normal_length_loss(dev):
    """the Eikonal term into every parameter, against float64; no warning: nothing takes the torch route"""
    from iso_points_amd import sdf_models
    from iso_points_amd.loss import NormalLengthLoss
    build = lambda: make_net(*SKIPPED, seed=121)      # noqa: E731
    pts = make_points(2 * 150, seed=122)
    m = build().to(dev)
    p = pts.reshape(2, 150, 3).to(dev)
    sdf_models._TORCH_WARNED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        normals, sdf = sdf_models.get_normals_from_grad(m, p, requires_grad=False, return_sdf=True)
        f0, g0 = sdf_models.idr_sdf_and_grad(m, p)
        assert not normals.requires_grad and normals.shape == (2, 150, 3) and sdf.shape == (2, 150, 1)
        assert torch.equal(normals, g0) and torch.equal(sdf.detach().squeeze(-1), f0)
        normals = sdf_models.get_normals_from_grad(m, p, requires_grad=True)
        assert normals.requires_grad and normals.grad_fn is not None
        NormalLengthLoss()(normals).backward()
    got = {k: v.grad.detach().double().cpu() for k, v in m.named_parameters()}
    lossfn = lambda f, g: NormalLengthLoss()(g.reshape(2, 150, 3))      # noqa: E731
    refs = tuple({k: v for k, v in r.items() if k != "points"} for r in module_refs(build, pts, lossfn, dev))
    assert_rule(got, refs, "eikonal")
    with pytest.raises(ValueError):
        sdf_models.sdf_forward(m, p, c=torch.zeros(1, 8, device=dev))


def test_sdf_forward_sends_a_siren_to_siren_forward(dev):
    from iso_points_amd.sdf_models import sdf_forward, siren_forward
    from siren_backward_oracle import make_net as make_siren
    m = make_siren(64, 2, seed=161).to(dev)
    p = make_points(300, seed=162).to(dev)
    U, V = (t.to(dev) for t in seeded_UV(300, 161))
    outs = []
    for fn in (siren_forward, sdf_forward):
        mm = copy.deepcopy(m)
        x = p.clone().requires_grad_(True)
        f, g = fn(mm, x)
        ((U * f).sum() + (V * g).sum()).backward()
        outs.append([f.detach(), g.detach(), x.grad] + [v.grad for v in mm.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_three_sgd_steps_on_sdf_and_eikonal(dev):
    """Three plain SGD steps on mean(f^2) + 0.01 mean((|g| - 1)^2): the losses and the final parameters stay within the
    oracle rule's distance of float64, torch's float32 autograd on the CPU and the GPU being the comparison."""
    from iso_points_amd.sdf_models import idr_forward
    net = make_net(*SKIPPED, seed=141)
    pts = make_points(512, seed=142)
    lr = 1e-4

    def steps(dtype, device, fused=False):
        m = copy.deepcopy(net).to(dtype).to(device)
        p = pts.to(dtype).to(device)
        losses = []
        for _ in range(3):
            if fused:
                f, g = idr_forward(m, p)
            else:
                x = p.clone().requires_grad_(True)
                f = m(x).sdf.squeeze(-1)
                g = torch.autograd.grad(f.sum(), x, create_graph=True)[0]
            loss = (f ** 2).mean() + 0.01 * ((g.norm(dim=-1) - 1) ** 2).mean()
            grads = torch.autograd.grad(loss, list(m.parameters()))
            with torch.no_grad():
                for v, gr in zip(m.parameters(), grads):
                    v -= lr * gr
            losses.append(loss.detach())
        out = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
        out["losses"] = torch.stack(losses).double().cpu()
        return out
    refs = (steps(torch.float64, "cpu"), steps(torch.float32, "cpu"), steps(torch.float32, dev))
    moved = max((refs[0][k] - v.detach().double()).abs().max().item() for k, v in net.named_parameters())
    assert moved > 0
    assert_rule(steps(torch.float32, dev, fused=True), refs, "sgd")
