"""The texture network's backward (csrc/texgrad.hip, iso_texgrad_backward; texture._TextureFunction) against torch autograd
of the same module in float64 on the CPU.  Oracle, fence filter and criterion: tests/texture_backward_oracle.py.

The kernels are called directly (abi_grads: NaN-guarded inputs, NaN-filled outputs and workspace) where the effective
weights' gradients are looked at, and through texture_rgb and torch's backward (autograd_grads) where the parameters'
are.  BACKWARD_CASES is read by tests/test_texture_backward_cpu.py."""
import warnings

import pytest
import torch

from test_texture_gpu import CASES, KPAD, make_inputs, make_net, on_gpu
from texture_backward_oracle import (FACTOR, FLOOR, KEEP_AT_LEAST, abi_grads, assert_criterion, autograd_grads, err,
                                     fence_filter, references, seeded_G, torch_grads)

pytestmark = pytest.mark.gpu

N = 1500
FORMS = [(512, 4, 256, 6, 4), (512, 4, 0, 6, 4), (256, 1, 0, 3, -1), (512, 8, 256, 6, 6), (256, 8, 256, 6, 6), (512, 1, 8, 6, 0),
         (256, 4, 0, 3, 4)]
COUNTS_SHAPE = (256, 1, 8, 6, 4)
ROUNDS = [(256, 1, 8, 6, 4), (512, 1, 0, 6, 0)]
BACKWARD_CASES = FORMS + KPAD + [COUNTS_SHAPE] + ROUNDS
assert set(ROUNDS) <= set(CASES) and set(KPAD) <= set(CASES)


def _form(shape):
    from iso_points_amd import _lib
    assert _lib.load().iso_texgrad_form(*shape) == 700 + shape[0] // 16, shape


def filtered(shape, net, n, seed, n_clouds=1):
    """n points of make_inputs that pass the fence filter (at least 97 % of the drawn ones must)"""
    raw = make_inputs(shape, n + max(64, n // 16), seed, n_clouds=n_clouds)
    inp, kept = fence_filter(net, raw)
    assert kept >= KEEP_AT_LEAST, (shape, kept)
    assert inp[0].shape[0] >= n, (shape, kept)
    m = inp[0].shape[0]
    return tuple(t if (t is None or t.shape[0] != m or t is inp[3]) else t[:n].contiguous() for t in inp)


def run(shape, net, inp, dev, seed, what=None, G=None):
    _form(shape)
    G = seeded_G(inp[0].shape[0], seed) if G is None else G
    refs = references(net, inp, G, dev)
    got = abi_grads(net, inp, G, dev)
    assert_criterion(got, refs, what or (shape,))
    return got, refs


@pytest.mark.parametrize("shape", FORMS)
def test_forms(dev, shape):
    net = make_net(shape, seed=shape[1], weight_norm=False)
    run(shape, net, filtered(shape, net, N, seed=shape[2]), dev, seed=1)


@pytest.mark.parametrize("shape", KPAD)
def test_k_padding_of_layer_0(dev, shape):
    """dW_0 and the three input gradients slot by slot; d points is the oracle's with the direction detached, and the
    case can tell that from the oracle's without the detach."""
    H, NL, C, Gm, Fq = shape
    assert C + Gm + (3 + 6 * Fq if Fq >= 0 else 0) in (3, 63, 64, 65, 301)
    net = make_net(shape, seed=C, weight_norm=False)
    inp = filtered(shape, net, N, seed=C + 1)
    got, refs = run(shape, net, inp, dev, seed=2)
    assert got["W0"].shape == (H, C + Gm + (3 + 6 * Fq if Fq >= 0 else 0))
    assert got["points"].shape == (N, 3) and (C == 0 or got["codes"].shape == (N, C))
    if Fq >= 0:
        G = seeded_G(N, 2)
        free = torch_grads(net, inp, G, torch.float64, detach_view=False)["points"]
        g64, g32c, g32g = (r["points"] for r in refs)
        margin = FACTOR * max(err(g32c, g64), err(g32g, g64)) + FLOOR
        assert err(free, g64) > 100 * margin, (shape, err(free, g64), margin)
        assert err(got["points"], free) > 100 * margin, (shape, err(got["points"], free), margin)


def test_point_counts_around_the_partial_chunk(dev):
    from iso_points_amd import _lib
    chunk = _lib.load().iso_texgrad_chunk_points()
    assert chunk >= 64
    shape = COUNTS_SHAPE
    net = make_net(shape, seed=3)
    for n in (1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        run(shape, net, filtered(shape, net, n, seed=30 + n % 7), dev, seed=n, what=(shape, n))


@pytest.mark.parametrize("shape", ROUNDS)
def test_rounds_and_slices(dev, shape):
    """More points than one workspace chunk holds: the weight gradients against float64, and the same points in slices
    give the same bits in their rows: no point's arithmetic depends on its neighbours."""
    from iso_points_amd import _lib
    n = 256 * 64 + 65
    assert n > _lib.load().iso_texgrad_workspace_points()          # the second workspace chunk adds onto the first
    net = make_net(shape, seed=7)
    inp = filtered(shape, net, n, seed=8)
    G = seeded_G(n, 4)
    full, _ = run(shape, net, inp, dev, seed=4, what=(shape, n), G=G)
    for lo, hi in ((0, 1), (0, 64), (0, 65), (100, 230), (n - 65, n)):
        part = tuple(t if (t is None or t.shape[0] != n) else t[lo:hi].contiguous() for t in inp)
        got = abi_grads(net, part, G[lo:hi].contiguous(), dev)
        for k in ("points", "normals", "codes"):
            if k in full:
                assert torch.equal(got[k], full[k][lo:hi]), (shape, lo, hi, k)


def test_one_live_point(dev):
    shape = (256, 2, 8, 6, 4)
    net = make_net(shape, seed=9)
    inp = filtered(shape, net, N, seed=10)
    G = torch.zeros(N, 3)
    G[777] = torch.tensor([0.7, -1.3, 0.4])
    got, refs = run(shape, net, inp, dev, seed=0, what="one live point", G=G)
    others = torch.arange(N) != 777
    for k in ("points", "normals", "codes"):
        assert (got[k][others] == 0).all() and got[k][777].abs().max() > 0, k
    assert refs[0]["W1"].abs().max() > 0


def test_range_weights_times_50(dev):
    """tanh saturates: the gradients are at or near 0; they must be finite and within the margin."""
    shape = (256, 4, 8, 6, 4)
    net = make_net(shape, seed=9, weight_norm=False)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(50.0)
    run(shape, net, filtered(shape, net, N, seed=10), dev, seed=5, what="weights x 50")


def test_range_codes_times_1000(dev):
    shape = (512, 4, 256, 6, 4)
    net = make_net(shape, seed=12, weight_norm=False)
    pts, nrm, c, cams, idx = make_inputs(shape, N + 100, seed=11)
    inp, kept = fence_filter(net, (pts, nrm, c * 1.0e3, cams, idx))
    assert kept >= KEEP_AT_LEAST
    run(shape, net, tuple(t if t is inp[3] or t is None else t[:N].contiguous() for t in inp), dev, seed=6, what="codes x 1e3")


@pytest.mark.parametrize("shape", [(256, 2, 0, 6, 4), (512, 2, 8, 6, 0)])
def test_point_at_its_camera_centre(dev, shape):
    net = make_net(shape, seed=14)
    pts, nrm, c, cams, idx = filtered(shape, net, 200, seed=13)
    pts[17] = cams[0]
    pts[199] = cams[0]
    inp, kept = fence_filter(net, (pts, nrm, c, cams, idx))
    assert inp[0].shape[0] >= 198
    at_centre = (inp[0] == cams[0]).all(dim=1)
    assert int(at_centre.sum()) >= 1                       # the filter kept a point that sits on its camera centre
    got, _ = run(shape, net, inp, dev, seed=7, what=(shape, "at the centre"))
    assert all(torch.isfinite(v).all() for v in got.values())
    assert torch.isfinite(got["points"][at_centre]).all() and torch.isfinite(got["normals"][at_centre]).all()


def test_several_clouds(dev):
    shape = (256, 3, 8, 6, 4)
    net = make_net(shape, seed=15)
    inp = filtered(shape, net, N, seed=16, n_clouds=3)
    sizes = torch.bincount(inp[4].long(), minlength=3)
    assert sizes.min() > 0 and len(set(sizes.tolist())) == 3
    run(shape, net, inp, dev, seed=8, what="three clouds")


def test_two_calls_give_identical_bits(dev):
    shape = (512, 4, 256, 6, 4)
    net = make_net(shape, seed=17)
    inp = make_inputs(shape, 3000, seed=18)
    G = seeded_G(3000, 9)
    _form(shape)
    a, b = abi_grads(net, inp, G, dev), abi_grads(net, inp, G, dev)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- the autograd function ---------------------------------------------------------------------------------------------
def test_requires_grad_subsets(dev):
    from iso_points_amd.texture import PackedTexture, texture_rgb
    shape = (256, 2, 8, 6, 4)
    net = make_net(shape, seed=19)
    inp = filtered(shape, net, 300, seed=20)
    G = seeded_G(300, 10)
    refs = references(net, inp, G, dev)
    full = autograd_grads(net, inp, G, dev)
    assert_criterion(full, refs, "all")
    net = net.to(dev)
    pts, nrm, c, cams, idx = [on_gpu(t, dev) for t in inp]
    Gd = on_gpu(G, dev)
    # weights only
    net.zero_grad(set_to_none=True)
    rgb = texture_rgb(net, pts, nrm, c, cams, idx)
    assert rgb.grad_fn is not None
    (rgb * Gd).sum().backward()
    for k, v in net.named_parameters():
        assert torch.equal(v.grad.cpu(), full[k]), k
    # inputs only
    net.zero_grad(set_to_none=True)
    for v in net.parameters():
        v.requires_grad_(False)
    leaves = [t.clone().requires_grad_(True) for t in (pts, nrm, c)]
    rgb = texture_rgb(net, leaves[0], leaves[1], leaves[2], cams, idx)
    (rgb * Gd).sum().backward()
    for k, t in zip(("points", "normals", "codes"), leaves):
        assert torch.equal(t.grad.cpu(), full[k]), k
    assert all(v.grad is None for v in net.parameters())
    # nothing requires grad | no_grad | a caller's image
    assert texture_rgb(net, pts, nrm, c, cams, idx).grad_fn is None
    for v in net.parameters():
        v.requires_grad_(True)
    with torch.no_grad():
        plain = texture_rgb(net, pts, nrm, c, cams, idx)
    assert plain.grad_fn is None and not plain.requires_grad
    held = texture_rgb(net, leaves[0], leaves[1], leaves[2], cams, idx, packed=PackedTexture(net, dev))
    assert held.grad_fn is None and torch.equal(held, plain)
    assert torch.equal(texture_rgb(net, pts, nrm, c, cams, idx).detach(), plain)


@pytest.mark.parametrize("style", ["old", "parametrization", "plain"])
def test_weight_norm_styles(dev, style):
    import torch.nn as nn
    shape = (256, 2, 8, 6, 4)
    net = make_net(shape, seed=21, weight_norm=(style == "old"))
    if style == "parametrization":
        for l in range(net.num_layers - 1):
            nn.utils.parametrizations.weight_norm(getattr(net, "lin%d" % l))
    names = [k for k, _ in net.named_parameters()]
    assert any(("weight_g" in k) if style == "old" else ("original0" in k) if style == "parametrization" else k.endswith(".weight")
               for k in names)
    inp = filtered(shape, net, N, seed=22)
    G = seeded_G(N, 11)
    refs = references(net, inp, G, dev)
    got = autograd_grads(net, inp, G, dev)
    assert sorted(got) == sorted(k for k in refs[0] if not (k[0] in "Wb" and k[1:].isdigit()))
    assert_criterion(got, refs, style)


def test_neural_texture_branches_under_grad(dev):
    from iso_points_amd.texture import NeuralTexture
    lens = [300, 500, 200]
    cams3 = torch.randn(3, 3, generator=torch.Generator().manual_seed(19)) * 2
    for shape, view_dependent, use_cams in (((256, 2, 0, 3, -1), False, False), ((256, 2, 8, 6, -1), True, False),
                                            ((256, 2, 8, 6, 4), True, True)):
        _form(shape)
        net = make_net(shape, seed=20)
        pts, nrm, c, _, _ = make_inputs(shape, sum(lens), seed=21)
        idx = torch.repeat_interleave(torch.arange(3), torch.tensor(lens))
        cams = cams3 if use_cams else None
        inp, kept = fence_filter(net, (pts, nrm, c, cams, idx if use_cams else None))
        assert kept >= KEEP_AT_LEAST
        n = inp[0].shape[0]
        idx_kept = inp[4]
        G = seeded_G(n, 12)
        refs = references(net, inp, G, dev)
        tex = NeuralTexture(net.to(dev), view_dependent=view_dependent)
        p, nn_, cc = [None if t is None else on_gpu(t, dev).requires_grad_(True) for t in inp[:3]]
        rgb = tex(p, nn_, c=cc, camera_centers=cams3.to(dev) if use_cams else None,
                  cloud_idx=None if idx_kept is None else idx_kept.to(dev))
        assert rgb.grad_fn is not None
        (rgb * G.to(dev)).sum().backward()
        got = {k: v.grad.cpu() for k, v in net.named_parameters()}
        got.update({k: t.grad.cpu() for k, t in (("points", p), ("normals", nn_), ("codes", cc)) if t is not None})
        assert_criterion(got, refs, (shape, view_dependent))


def test_one_sgd_step_lowers_the_loss(dev):
    from iso_points_amd.texture import texture_rgb
    shape = (256, 2, 8, 6, 4)
    net = make_net(shape, seed=23).to(dev)
    pts, nrm, c, cams, idx = [None if t is None else t.to(dev) for t in make_inputs(shape, 1000, seed=24)]
    target = torch.rand(1000, 3, generator=torch.Generator().manual_seed(25)).to(dev)
    loss = lambda: ((texture_rgb(net, pts, nrm, c, cams, idx) - target) ** 2).mean()      # noqa: E731
    first = loss()
    before = first.detach().clone()
    rgb0 = texture_rgb(net, pts, nrm, c, cams, idx).detach()
    first.backward()
    with torch.no_grad():
        for p in net.parameters():
            p -= 0.05 * p.grad
    after = loss().detach()
    assert after.item() < before.item(), (before.item(), after.item())
    assert (texture_rgb(net, pts, nrm, c, cams, idx).detach() - rgb0).abs().max().item() > 1e-5


def test_unsupported_width_trains_on_torch_with_one_warning(dev):
    from iso_points_amd import _lib, texture as T
    shape = (128, 2, 8, 6, 4)
    assert _lib.load().iso_texgrad_form(*shape) == -1
    net = make_net(shape, seed=22).to(dev)
    pts, nrm, c, cams, idx = [None if t is None else t.to(dev) for t in make_inputs(shape, 300, seed=23)]
    G = seeded_G(300, 13).to(dev)
    T._TORCH_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        leaves = [t.clone().requires_grad_(True) for t in (pts, nrm, c)]
        (T.texture_rgb(net, leaves[0], leaves[1], leaves[2], cams) * G).sum().backward()
        T.texture_rgb(net, pts, nrm, c, cams)
    assert len([w for w in rec if "no fused texture kernel" in str(w.message)]) == 1
    got = {k: v.grad.clone() for k, v in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    want = [t.clone().requires_grad_(True) for t in (pts, nrm, c)]
    (net(T.texture_rows(net, want[0], want[1], cams), c=want[2]).rgb * G).sum().backward()
    for k, v in net.named_parameters():
        assert torch.equal(got[k], v.grad), k
    for a, b in zip(leaves, want):
        assert torch.equal(a.grad, b.grad)


# ---- refusals through the C ABI ----------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing(dev):
    from iso_points_amd import _lib
    lib = _lib.load()
    shape = (256, 2, 8, 6, 4)
    n = 100
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)       # noqa: E731
    pts, nrm, codes, cams, g = f(n, 3), f(n, 3), f(n, 8), f(1, 3), f(n, 3)
    packed = f(lib.iso_texgrad_packed_floats(*shape))
    packed_fw = f(lib.iso_texture_packed_floats(*shape))
    raw_n = lib.iso_texture_raw_floats(*shape)
    outs = dict(g_raw=nan(raw_n), g_pts=nan(n, 3), g_nrm=nan(n, 3), g_codes=nan(n, 8))
    ws = torch.zeros((lib.iso_texgrad_workspace_bytes(n, *shape),), dtype=torch.uint8, device=dev)
    P = _lib.ptr
    OK, INVALID, UNSUPPORTED = 0, -1, -2

    def call(shape=shape, pts=pts, nrm=nrm, codes=codes, cams=cams, idx=None, n_origins=1, g=g, n=n, packed=packed, packed_fw=packed_fw, ws=ws,
             ws_bytes=None, g_raw=outs["g_raw"], g_pts=outs["g_pts"], g_nrm=outs["g_nrm"], g_codes=outs["g_codes"]):
        return lib.iso_texgrad_backward(P(pts), P(nrm), P(codes), P(cams), P(idx), n_origins, P(g), n, P(packed_fw), P(packed), *shape, P(g_raw),
                                        P(g_pts), P(g_nrm), P(g_codes), P(ws), ws.numel() if ws_bytes is None else ws_bytes, None)
    for bad in ((128, 2, 8, 6, 4), (384, 2, 8, 6, 4), (256, 0, 8, 6, 4), (256, 9, 8, 6, 4), (256, 2, 257, 6, 4),
                (256, 2, -1, 6, 4), (256, 2, 8, 4, 4), (256, 2, 8, 6, 7), (256, 2, 8, 6, -2)):
        assert lib.iso_texgrad_form(*bad) == -1
        assert call(shape=bad) == UNSUPPORTED, bad
        assert lib.iso_texgrad_pack_weights(P(pts), P(packed), *bad, None) == UNSUPPORTED, bad
    assert b"iso_texgrad" in lib.iso_last_error()
    for kw in (dict(pts=None), dict(nrm=None), dict(codes=None), dict(cams=None), dict(g=None), dict(packed=None),
               dict(packed_fw=None), dict(ws=None, ws_bytes=1 << 30), dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0),
               dict(n_origins=0), dict(n=-1)):
        assert call(**kw) == INVALID, kw
    # a pointer where none is allowed
    assert call(shape=(256, 2, 8, 3, 4)) == INVALID and call(shape=(256, 2, 0, 6, 4)) == INVALID
    assert call(shape=(256, 2, 8, 6, -1)) == INVALID
    assert call(shape=(256, 2, 8, 3, 4), nrm=None) == INVALID              # grad_normals without normals
    assert lib.iso_texgrad_pack_weights(None, P(packed), *shape, None) == INVALID
    assert lib.iso_texgrad_pack_weights(P(pts), None, *shape, None) == INVALID
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs.values())                # nothing was written
    # grad_raw_out NULL: the weight gradients are not wanted, the input gradients are written
    assert call(g_raw=None) == OK
    torch.cuda.synchronize()
    assert torch.isnan(outs["g_raw"]).all() and all(torch.isfinite(outs[k]).all() for k in ("g_pts", "g_nrm", "g_codes"))
    # n == 0: zeros in grad_raw_out, whatever the other pointers
    assert lib.iso_texgrad_backward(None, None, None, None, None, 0, None, 0, None, None, *shape, P(outs["g_raw"]), None, None, None,
                                    None, 0, None) == OK
    torch.cuda.synchronize()
    assert float(outs["g_raw"].abs().max()) == 0.0
