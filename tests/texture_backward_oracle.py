"""Shared by the texture-backward tests: the float64 oracle (torch autograd of the module on the CPU, loss sum(rgb * G) with
a seeded G), the fence filter on the inputs, the two float32 comparison runs and the criterion.

Fence filter: a ReLU mask flips when z is within rounding of 0, in any float32 path, so a point is kept iff every hidden
pre-activation has |z64_l[k]| >= 1e-6 max|z64_l|; the inputs are filtered BEFORE anyone computes a gradient.

Criterion, per gradient tensor: e = max|grad - grad64| / max|grad64|, e_hip <= 1.5 max(e_cpu, e_gpu) + 2e-7, e_cpu / e_gpu
being the same module in float32 on the CPU / eagerly on the test's GPU."""
import copy

import torch
import torch.nn.functional as F

from test_texture_gpu import clone_net, on_gpu

FENCE = 1e-6
KEEP_AT_LEAST = 0.97
FACTOR, FLOOR = 1.5, 2e-7


def rows_of(m, p, nrm, cams, idx, detach_view=True):
    """texture_rows, with the detach of the direction (texture.py:152) as a switch"""
    x = p if nrm is None else torch.cat([nrm, p], dim=-1)
    if cams is not None:
        cam = cams[idx.long()] if idx is not None else cams[:1]
        view = F.normalize((p.detach() if detach_view else p) - cam, dim=-1)
        if m.embed_fn is not None:
            view = m.embed_fn(view)
        x = torch.cat([x, view], dim=-1)
    return x


def clone_any(net, dtype):
    """CPU copy in dtype: clone_net for plain / old-style weight-norm, deepcopy for the parametrization"""
    if hasattr(net.lin0, "parametrizations"):
        return copy.deepcopy(net).cpu().to(dtype)
    return clone_net(net, dtype)


def n_hidden(m):
    return m.num_layers - 2


def fence_filter(net, inp):
    """inp restricted to the points every hidden pre-activation of which is off the fence; the kept fraction"""
    pts, nrm, c, cams, idx = inp
    m = clone_any(net, torch.float64)
    with torch.no_grad():
        x = rows_of(m, pts.double(), None if nrm is None else nrm.double(), None if cams is None else cams.double(), idx)
        if c is not None:
            x = torch.cat([c.double(), x], dim=-1)
        keep = torch.ones(pts.shape[0], dtype=torch.bool)
        for l in range(n_hidden(m)):
            z = getattr(m, "lin%d" % l)(x)
            keep &= (z.abs() >= FENCE * z.abs().max()).all(dim=1)
            x = torch.relu(z)
    n = pts.shape[0]
    out = tuple(t if (t is None or t.shape[0] != n or t is cams) else t[keep].contiguous() for t in inp)
    return out, keep.float().mean().item()


def seeded_G(n, seed):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(5000 + seed))


def torch_grads(net, inp, G, dtype, device="cpu", detach_view=True):
    """{name: float64 CPU gradient}: every parameter of the module by its own name, the effective weights and biases as
    W0.., b0.. (plain and old-style weight-norm), points / normals / codes"""
    pts, nrm, c, cams, idx = inp
    m = clone_any(net, dtype).to(device)
    leaf = lambda t: None if t is None else t.detach().clone().to(dtype).to(device).requires_grad_(True)      # noqa: E731
    p, nn_, cc = leaf(pts), leaf(nrm), leaf(c)
    cam = None if cams is None else cams.to(dtype).to(device)
    ix = None if idx is None else idx.to(device)
    rgb = m(rows_of(m, p, nn_, cam, ix, detach_view), c=cc).rgb
    eff = []
    if not hasattr(m.lin0, "parametrizations"):
        for l in range(m.num_layers - 1):
            w = getattr(m, "lin%d" % l).weight
            w.retain_grad()
            eff.append(w)
    (rgb * G.to(dtype).to(device)).sum().backward()
    out = {k: v.grad.detach().double().cpu() for k, v in m.named_parameters()}
    for l, w in enumerate(eff):
        out["W%d" % l] = w.grad.detach().double().cpu()
        out["b%d" % l] = getattr(m, "lin%d" % l).bias.grad.detach().double().cpu()
    for k, t in (("points", p), ("normals", nn_), ("codes", cc)):
        if t is not None:
            out[k] = t.grad.detach().double().cpu()
    return out


def err(g, g64):
    top = g64.abs().max().item()
    d = (g.double() - g64).abs().max().item()
    return d / top if top > 0 else d


def assert_criterion(got, refs, what, keys=None):
    """got: {name: tensor}; refs = (g64, g32_cpu, g32_gpu)"""
    g64, g32c, g32g = refs
    for k in (keys if keys is not None else sorted(got)):
        assert torch.isfinite(got[k]).all(), "%s %s: non-finite gradient" % (what, k)
        assert got[k].shape == g64[k].shape, (what, k, got[k].shape, g64[k].shape)
        e_hip, e_cpu, e_gpu = err(got[k], g64[k]), err(g32c[k], g64[k]), err(g32g[k], g64[k])
        print("%s %s: e_cpu %.3g e_gpu %.3g e_hip %.3g" % (what, k, e_cpu, e_gpu, e_hip))
        assert e_hip <= FACTOR * max(e_cpu, e_gpu) + FLOOR, (what, k, e_cpu, e_gpu, e_hip)


def references(net, inp, G, dev, detach_view=True):
    return (torch_grads(net, inp, G, torch.float64, "cpu", detach_view), torch_grads(net, inp, G, torch.float32, "cpu", detach_view),
            torch_grads(net, inp, G, torch.float32, dev, detach_view))


def nan_like(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def abi_grads(net, inp, G, dev, want=("points", "normals", "codes")):
    """iso_texgrad_backward called directly on the module's effective weights: every input a slice of a NaN-filled buffer,
    every output and the workspace pre-filled with NaN.  Returns {W0.., b0.., points, normals, codes} on the CPU."""
    from iso_points_amd import _lib
    from iso_points_amd.texture import texture_spec
    lib = _lib.load()
    Ws, bs, H, NL, C, Gm, Fq = texture_spec(net)
    shape = (H, NL, C, Gm, Fq)
    assert lib.iso_texgrad_form(*shape) == 700 + H // 16, shape
    pts, nrm, c, cams, idx = inp
    n = pts.shape[0]
    wb = [t for pair in zip(Ws, bs) for t in pair]
    raw = on_gpu(torch.cat([t.detach().reshape(-1).float().cpu() for t in wb]), dev)
    assert raw.numel() == lib.iso_texture_raw_floats(*shape)
    packed = nan_like((lib.iso_texgrad_packed_floats(*shape),), dev)
    _lib.call("iso_texgrad_pack_weights", _lib.ptr(raw), _lib.ptr(packed), *shape, _lib.stream())
    packed_fw = nan_like((lib.iso_texture_packed_floats(*shape),), dev)
    _lib.call("iso_texture_pack_weights", _lib.ptr(raw), _lib.ptr(packed_fw), *shape, _lib.stream())
    d = [on_gpu(t, dev) for t in (pts, nrm, c, cams, None if idx is None else idx.to(torch.int32), G)]
    g_raw = nan_like((raw.numel(),), dev)
    g_pts = nan_like((n, 3), dev) if "points" in want else None
    g_nrm = nan_like((n, 3), dev) if ("normals" in want and nrm is not None) else None
    g_c = nan_like((n, C), dev) if ("codes" in want and c is not None) else None
    ws = nan_like((lib.iso_texgrad_workspace_bytes(n, *shape) // 4,), dev)
    _lib.call("iso_texgrad_backward", _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]),
              0 if cams is None else cams.shape[0], _lib.ptr(d[5]), n, _lib.ptr(packed_fw), _lib.ptr(packed), *shape,
              _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(g_nrm), _lib.ptr(g_c), _lib.ptr(ws), ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    out, at = {}, 0
    g_raw = g_raw.cpu()
    for l, (W, b) in enumerate(zip(Ws, bs)):
        out["W%d" % l] = g_raw[at:at + W.numel()].reshape(W.shape)
        at += W.numel()
        out["b%d" % l] = g_raw[at:at + b.numel()]
        at += b.numel()
    for k, t in (("points", g_pts), ("normals", g_nrm), ("codes", g_c)):
        if t is not None:
            out[k] = t.cpu()
    return out


def autograd_grads(net, inp, G, dev):
    """Through texture_rgb and torch's backward: {parameter name: grad, points, normals, codes} on the CPU"""
    from iso_points_amd.texture import texture_rgb
    net = net.to(dev)
    net.zero_grad(set_to_none=True)
    pts, nrm, c, cams, idx = [on_gpu(t, dev) for t in inp]
    for t in (pts, nrm, c):
        if t is not None:
            t.requires_grad_(True)
    rgb = texture_rgb(net, pts, nrm, c, cams, idx)
    assert rgb.grad_fn is not None
    (rgb * on_gpu(G, dev)).sum().backward()
    torch.cuda.synchronize()
    out = {k: v.grad.detach().cpu() for k, v in net.named_parameters()}
    for k, t in (("points", pts), ("normals", nrm), ("codes", c)):
        if t is not None:
            out[k] = t.grad.detach().cpu()
    return out
