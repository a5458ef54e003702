"""The SIREN SDF's backward (csrc/sirengrad.hip, iso_sirengrad_backward; sdf_models._SirenFunction / siren_forward /
get_normals_from_grad) against torch's double backward of the same module in float64 on the CPU.  Oracle and criterion:
tests/siren_backward_oracle.py.

The kernels are called directly (abi_grads: NaN-guarded inputs, NaN-filled outputs and workspace) where the effective
weights' gradients are looked at, and through siren_forward and torch's backward where the parameters' are.
BACKWARD_CASES (model width, hidden layers, tangent form) is read by tests/test_siren_backward_cpu.py."""
import copy
import ctypes
import warnings

import pytest
import torch

from siren_backward_oracle import (FACTOR, FLOOR, abi_grads, assert_criterion, err, make_net, make_points, nan_like, on_gpu,
                                   padded_raw, references, seeded_UV)

pytestmark = pytest.mark.gpu

N = 1000
FORMS = [(H, L) for H in (64, 128, 256) for L in (0, 1, 3)] + [(64, 8)]
PADDED = [(48, 2), (200, 2)]
COUNTS_SHAPE = (64, 1)
VALUE_ONLY = [(64, 1), (128, 2), (256, 1)]
BACKWARD_CASES = [(H, L, True) for H, L in FORMS + PADDED + [COUNTS_SHAPE]] + [(H, L, False) for H, L in VALUE_ONLY]


def run(shape, n, dev, seed, U=None, V="seeded", scale=1.0, what=None):
    H, L = shape
    net = make_net(H, L, seed=seed)
    pts = make_points(n, seed=seed + 1, scale=scale)
    sU, sV = seeded_UV(n, seed)
    U = sU if U is None else U
    V = sV if isinstance(V, str) else V
    refs = references(net, pts, U, V, dev)
    got = abi_grads(net, pts, U, V, dev)
    assert_criterion(got, refs, what or (shape, n), L)
    return net, pts, U, V, got, refs


@pytest.mark.parametrize("shape", FORMS)
def test_forms_and_depths(dev, shape):
    run(shape, N, dev, seed=shape[0] + shape[1])


@pytest.mark.parametrize("shape", PADDED)
def test_padded_widths(dev, shape):
    """a width other than 64 / 128 / 256 runs as the next one up; the added rows and columns get zero gradients (abi_grads)"""
    net, pts, U, V, got, _ = run(shape, N, dev, seed=shape[0])
    assert got["W1"].shape == (shape[0], shape[0]) and got["W0"].shape == (shape[0], 3)


def test_point_counts_around_the_tile_and_the_partial_chunk(dev):
    from iso_points_amd import _lib
    chunk = _lib.load().iso_sirengrad_chunk_points()
    assert chunk >= 66
    for n in (1, 7, 8, 9, 63, 64, 65, chunk - 1, chunk, chunk + 1):
        run(COUNTS_SHAPE, n, dev, seed=n)


def test_two_workspace_chunks_and_slices(dev):
    """More points than one workspace chunk holds: the weight gradients against float64 (the second chunk adds onto the
    first), and the same points run alone give the same bits in their rows of d points."""
    from iso_points_amd import _lib
    wsp = _lib.load().iso_sirengrad_workspace_points()
    n = wsp + 37
    net, pts, U, V, full, _ = run(COUNTS_SHAPE, n, dev, seed=11)
    for lo, hi in ((0, 1), (0, 33), (100, 230), (wsp - 5, wsp), (wsp, n), (wsp - 40, wsp + 9)):
        got = abi_grads(net, pts[lo:hi].contiguous(), U[lo:hi].contiguous(), V[lo:hi].contiguous(), dev, want_raw=False)
        assert torch.equal(got["points"], full["points"][lo:hi]), (lo, hi)


@pytest.mark.parametrize("shape", VALUE_ONLY)
def test_value_only_is_the_first_order_backward(dev, shape):
    """v absent: the gradient of sum(U f) alone, on the form without tangent columns"""
    net, pts, U, V, got, refs = run(shape, N, dev, seed=21 + shape[1], V=None)
    # ... and it is not the tangent form run on v = 0 by accident of the dispatch: that gives the same mathematics
    zero = abi_grads(net, pts, U, torch.zeros(N, 3), dev)
    assert_criterion(zero, refs, (shape, "v = 0"), shape[1])


def test_gradient_only(dev):
    run((128, 2), N, dev, seed=31, U=torch.zeros(N))


def test_one_live_point(dev):
    n, live = 700, 333
    U, V = torch.zeros(n), torch.zeros(n, 3)
    sU, sV = seeded_UV(n, 41)
    U[live], V[live] = sU[live], sV[live]
    net, pts, U, V, got, refs = run((64, 2), n, dev, seed=41, U=U, V=V)
    dead = torch.ones(n, dtype=torch.bool)
    dead[live] = False
    assert (got["points"][dead] == 0).all() and got["points"][live].abs().max() > 0


@pytest.mark.parametrize("scale", [1e-3, 3.0])
def test_scaled_points(dev, scale):
    """the arguments of layer 0's sine: tiny, and several periods"""
    run((128, 1), N, dev, seed=51, scale=scale)


def test_two_calls_give_the_same_bits(dev):
    net = make_net(128, 2, seed=61)
    n = 2 * 256 + 77
    pts = make_points(n, seed=62)
    U, V = seeded_UV(n, 61)
    a, b = abi_grads(net, pts, U, V, dev), abi_grads(net, pts, U, V, dev)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_null_outputs_select_the_work(dev):
    """grad_raw_out NULL: d points alone, the same bits; grad_pts_out NULL: the weight gradients alone, the same bits; both
    NULL: nothing is launched and the workspace stays as it was"""
    from iso_points_amd import _lib
    lib = _lib.load()
    net = make_net(64, 2, seed=71)
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
    raw_cpu, H = padded_raw(net)
    raw = raw_cpu.to(dev)
    packed = torch.empty((lib.iso_siren_packed_floats(H, 2),), dtype=torch.float32, device=dev)
    _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, 2, _lib.stream())
    ws = nan_like((lib.iso_sirengrad_workspace_bytes(n, H, 2) // 4,), dev)
    d_pts, d_u, d_v = pts.to(dev), U.to(dev), V.to(dev)
    _lib.call("iso_sirengrad_backward", _lib.ptr(d_pts), _lib.ptr(d_u), _lib.ptr(d_v), n, _lib.ptr(raw),
              _lib.ptr(packed), H, 2, 30.0, 30.0, None, None, _lib.ptr(ws), ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()
    # the entry with a tail of layer 0's bias: a tail of zeros is the plain call, bit for bit
    g_raw, g_pts, tail = nan_like((raw.numel(),), dev), nan_like((n, 3), dev), torch.zeros(H, device=dev)
    _lib.call("iso_sirengrad_backward_b0", _lib.ptr(d_pts), _lib.ptr(d_u), _lib.ptr(d_v), n, _lib.ptr(raw), _lib.ptr(packed), H, 2,
              30.0, 30.0, _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(ws), ws.numel() * 4, _lib.stream(), _lib.ptr(tail))
    torch.cuda.synchronize()
    assert torch.equal(g_pts.cpu(), full["points"])
    assert torch.equal(g_raw.cpu()[:192].reshape(64, 3), full["W0"]) and torch.equal(g_raw.cpu()[-65:-1].reshape(1, 64), full["W3"])


# ---- through siren_forward and torch's backward ---------------------------------------------------------------------------
def module_grads(model, pts, c, lossfn, dtype, device, fused=False):
    """{parameter name: grad, points, code} as float64 CPU tensors of lossfn(f, g); fused: through siren_forward"""
    from iso_points_amd.sdf_models import siren_forward
    m = copy.deepcopy(model).to(dtype).to(device)
    p = (on_gpu(pts, device) if fused else pts.to(dtype).to(device)).detach().requires_grad_(True)
    cc = None if c is None else c.detach().clone().to(dtype).to(device).requires_grad_(True)
    if fused:
        f, g = siren_forward(m, p, c=cc)
        assert f.grad_fn is not None and g.grad_fn is not None
    else:
        x = p if cc is None else torch.cat([cc.reshape(1, -1).expand(p.shape[0], -1), p], dim=-1)
        f = (m.net(x) if hasattr(m, "net") else m(x).sdf).squeeze(-1)
        g = torch.autograd.grad(f.sum(), p, create_graph=True)[0]
    lossfn(f, g).backward()
    if device != "cpu":
        torch.cuda.synchronize()
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().double().cpu() for k, v in m.named_parameters()}
    out["points"] = p.grad.detach().double().cpu()
    if cc is not None:
        out["code"] = cc.grad.detach().double().cpu()
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


def module_refs(model, pts, c, lossfn, dev):
    return (module_grads(model, pts, c, lossfn, torch.float64, "cpu"), module_grads(model, pts, c, lossfn, torch.float32, "cpu"),
            module_grads(model, pts, c, lossfn, torch.float32, dev))


@pytest.mark.parametrize("which", ["oracle_module", "reference_layout"])
def test_siren_forward_trains_every_parameter(dev, which):
    from iso_points_amd.sdf_models import Siren
    if which == "oracle_module":
        model = make_net(128, 2, seed=81)
    else:
        with torch.random.fork_rng():
            torch.manual_seed(82)
            model = Siren(hidden_size=64, n_layers=2)
    pts = make_points(600, seed=83)
    lossfn = uv_loss(*seeded_UV(600, 81))
    got = module_grads(model, pts, None, lossfn, torch.float32, dev, fused=True)
    assert_rule(got, module_refs(model, pts, None, lossfn, dev), which)


def test_requires_grad_subsets(dev):
    """only the points; only the weights; only one layer's bias: what needs no gradient gets none, the rest is unchanged"""
    from iso_points_amd.sdf_models import siren_forward
    net = make_net(64, 2, seed=91).to(dev)
    pts = make_points(300, seed=92).to(dev)
    U, V = (t.to(dev) for t in seeded_UV(300, 91))

    def grads(p_grad, names):
        m = copy.deepcopy(net)
        for k, v in m.named_parameters():
            v.requires_grad_(names is None or k in names)
        p = pts.clone().requires_grad_(p_grad)
        f, g = siren_forward(m, p)
        ((U * f).sum() + (V * g).sum()).backward()
        out = {k: v.grad for k, v in m.named_parameters()}
        out["points"] = p.grad
        return out
    full = grads(True, None)
    assert all(v is not None for v in full.values())
    for p_grad, names in ((True, ()), (False, None), (False, ("lins.1.bias",))):
        got = grads(p_grad, names)
        for k, v in got.items():
            wanted = p_grad if k == "points" else (names is None or k in names)
            assert (v is not None) == wanted, (p_grad, names, k)
            if wanted:
                assert torch.equal(v, full[k]), (p_grad, names, k)


def test_one_code_latent_siren(dev):
    """c_dim = 8, one code for all points: d code and the code columns of W_0 come from torch's chain over the fused
    backward's effective b_0; all against float64"""
    from iso_points_amd.sdf_models import Siren
    with torch.random.fork_rng():
        torch.manual_seed(101)
        model = Siren(hidden_size=64, n_layers=2, c_dim=8)
        c = torch.randn(1, 8) * 0.3
    pts = make_points(500, seed=102)
    lossfn = uv_loss(*seeded_UV(500, 101))
    got = module_grads(model, pts, c, lossfn, torch.float32, dev, fused=True)
    refs = module_refs(model, pts, c, lossfn, dev)
    assert got["code"].shape == (1, 8) and got["net.0.linear.weight"].shape == (64, 11)
    assert refs[0]["net.0.linear.weight"][:, :8].abs().max() > 0
    assert_rule(got, refs, "latent")


def test_per_row_codes_take_the_torch_route_with_a_warning(dev):
    from iso_points_amd import sdf_models
    with torch.random.fork_rng():
        torch.manual_seed(111)
        model = sdf_models.Siren(hidden_size=64, n_layers=1, c_dim=8).to(dev)
        c = (torch.randn(2, 8) * 0.3).to(dev).requires_grad_(True)
    pts = make_points(100, seed=112).reshape(2, 50, 3).to(dev)
    sdf_models._TORCH_WARNED.clear()
    with pytest.warns(RuntimeWarning, match="one code per batch row"):
        f, g = sdf_models.siren_forward(model, pts, c=c)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                               # one warning per model class
        f2, _ = sdf_models.siren_forward(model, pts, c=c)
    assert f.shape == (2, 50) and g.shape == (2, 50, 3) and f.grad_fn is not None and g.grad_fn is not None
    want = model.forward(pts, c=c[:, None, :].expand(2, 50, 8)).sdf.squeeze(-1)
    assert torch.equal(f, want) and torch.equal(f2, want)
    ((f ** 2).sum() + (g ** 2).sum()).backward()
    assert c.grad is not None and torch.isfinite(c.grad).all() and c.grad.abs().max() > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_get_normals_from_grad_on_both_branches(dev):
    from iso_points_amd.loss import NormalLengthLoss
    from iso_points_amd.sdf_models import get_normals_from_grad, siren_sdf_and_grad
    model = make_net(64, 2, seed=121)
    pts = make_points(2 * 150, seed=122).reshape(2, 150, 3)
    m = copy.deepcopy(model).to(dev)
    p = pts.to(dev)
    # detached
    normals, sdf = get_normals_from_grad(m, p, requires_grad=False, return_sdf=True)
    f0, g0 = siren_sdf_and_grad(m, p)
    assert not normals.requires_grad and normals.shape == (2, 150, 3) and sdf.shape == (2, 150, 1)
    assert torch.equal(normals, g0) and torch.equal(sdf.detach().squeeze(-1), f0)
    assert not p.requires_grad
    assert torch.equal(get_normals_from_grad(m, p), g0)
    # training: the Eikonal term into every parameter, against float64
    lossfn = lambda f, g: NormalLengthLoss()(g)      # noqa: E731
    normals = get_normals_from_grad(m, p, requires_grad=True)
    assert normals.requires_grad and normals.grad_fn is not None
    NormalLengthLoss()(normals).backward()
    got = {k: v.grad.detach().double().cpu() for k, v in m.named_parameters()}
    assert "lins.3.bias" in got and got["lins.3.bias"].abs().max() == 0      # the head's bias does not move the normals
    flat = pts.reshape(-1, 3)
    refs = tuple({k: v for k, v in r.items() if k != "points"} for r in module_refs(model, flat, None, lossfn, dev))
    assert_rule(got, refs, "eikonal")


def test_siren_forward_without_grad_is_the_detached_route(dev, gemm_mode):
    from iso_points_amd.sdf_models import siren_forward, siren_sdf_and_grad
    m = make_net(128, 2, seed=131).to(dev)
    p = make_points(777, seed=132).to(dev)
    f0, g0 = siren_sdf_and_grad(m, p)
    with torch.no_grad():
        f1, g1 = siren_forward(m, p)
    for v in m.parameters():
        v.requires_grad_(False)
    f2, g2 = siren_forward(m, p)
    f3, g3 = siren_forward(m, p, need_grad=False)
    assert g3 is None and f1.grad_fn is None and f2.grad_fn is None
    for f, g in ((f1, g1), (f2, g2)):
        assert torch.equal(f, f0) and torch.equal(g, g0)
    assert torch.equal(f3, f0)
    # ... and under grad the values are the same evaluation's
    for v in m.parameters():
        v.requires_grad_(True)
    f4, g4 = siren_forward(m, p)
    assert f4.grad_fn is not None and torch.equal(f4.detach(), f0) and torch.equal(g4.detach(), g0)


def test_three_sgd_steps_on_sdf_and_eikonal(dev):
    """Three plain SGD steps on mean(f^2) + 0.01 mean((|g| - 1)^2): the losses and the final parameters stay within the
    oracle rule's distance of float64, torch's float32 autograd on the CPU and the GPU being the comparison."""
    from iso_points_amd.sdf_models import siren_forward
    net = make_net(64, 2, seed=141)
    pts = make_points(512, seed=142)
    lr = 1e-4

    def steps(dtype, device, fused=False):
        m = copy.deepcopy(net).to(dtype).to(device)
        p = pts.to(dtype).to(device)
        losses = []
        for _ in range(3):
            if fused:
                f, g = siren_forward(m, p)
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


# ---- every refusal of the entry point ----------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from iso_points_amd import _lib
    lib = _lib.load()
    H, L, n = 64, 1, 100
    net = make_net(H, L, seed=151)
    raw = padded_raw(net)[0].to(dev)
    packed = torch.empty((lib.iso_siren_packed_floats(H, L) + 4,), dtype=torch.float32, device=dev)
    _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, L, _lib.stream())
    pts, (U, V) = make_points(n, seed=152).to(dev), (t.to(dev) for t in seeded_UV(n, 151))
    need = lib.iso_sirengrad_workspace_bytes(n, H, L)
    ws = nan_like((need // 4 + 4,), dev)
    g_raw, g_pts = nan_like((raw.numel(),), dev), nan_like((n, 3), dev)
    P = _lib.ptr
    st = _lib.stream()

    def call(**kw):
        a = dict(pts=P(pts), u=P(U), v=P(V), n=n, raw=P(raw), packed=P(packed), H=H, L=L, g_raw=P(g_raw), g_pts=P(g_pts), ws=P(ws),
                 bytes=need)
        a.update(kw)
        return lib.iso_sirengrad_backward(a["pts"], a["u"], a["v"], a["n"], a["raw"], a["packed"], a["H"], a["L"], 30.0, 30.0,
                                          a["g_raw"], a["g_pts"], a["ws"], a["bytes"], st)
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    for H_bad in (0, 48, 63, 65, 96, 255, 257, 512):
        assert call(H=H_bad) == UNSUPPORTED, H_bad
    assert call(L=-1) == UNSUPPORTED and call(L=9) == UNSUPPORTED
    assert call(n=-1) == INVALID
    for k in ("pts", "u", "packed", "ws"):
        assert call(**{k: None}) == INVALID, k
    assert call(bytes=need - 1) == WORKSPACE and call(bytes=0) == WORKSPACE
    assert call(ws=ctypes.c_void_p(ws.data_ptr() + 4)) == INVALID
    assert call(packed=ctypes.c_void_p(packed.data_ptr() + 4)) == INVALID
    assert b"iso_sirengrad_backward" in lib.iso_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(g_raw).all() and torch.isnan(g_pts).all() and torch.isnan(ws).all()
    # n = 0: nothing to sum, zeros; the points' output is not touched
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (g_raw == 0).all() and torch.isnan(g_pts).all() and torch.isnan(ws).all()
    # and the accepted call right at the limits: n_hidden 8 is covered by the forms; the exact workspace size here
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(g_raw).all() and torch.isfinite(g_pts).all()
