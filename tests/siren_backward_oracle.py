"""Shared by the SIREN-backward tests: the float64 oracle (torch autograd of oracle.iso_oracle.SirenSDF on the CPU:
autograd.grad(create_graph=True) for g = grad_x f, then the backward of sum(U f) + sum(V . g) with seeded U, V), the
tangent-form formulas of DESIGN.md 3.1c restated in torch without autograd, the float32 comparison runs and the criterion.

Criterion (tests/texture_backward_oracle.py's), per gradient tensor: e = max|grad - grad64| / max|grad64|,
e_hip <= 1.5 max(e_cpu, e_gpu) + 2e-7, e_cpu / e_gpu being torch's own float32 double backward of the same module on the CPU
/ eagerly on the test's GPU.  A SIREN has no activation fence: no point is filtered out.

Gradient names: W0, b0 (layer 0), W1.. / b1.. (hidden layers), W{L+1}, b{L+1} (the head), points."""
import copy

import torch

from oracle.iso_oracle import SirenSDF

FACTOR, FLOOR = 1.5, 2e-7
WORST = {}          # tensor class -> worst e_hip / limit seen by assert_criterion in this process


def make_net(hidden, n_hidden, seed, w0=30.0, wh=30.0):
    with torch.random.fork_rng():
        torch.manual_seed(4000 + seed)
        return SirenSDF(hidden_size=hidden, n_layers=n_hidden, first_omega_0=w0, hidden_omega_0=wh)


def make_points(n, seed, scale=1.0):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(1000 + seed)) * 2 - 1) * scale


def seeded_UV(n, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn(n, generator=g), torch.randn(n, 3, generator=g)


def names_of(n_hidden):
    return [k + str(l) for l in range(n_hidden + 2) for k in ("W", "b")]


def class_of(name, n_hidden):
    if name == "points":
        return "dx"
    l = int(name[1:])
    if l == n_hidden + 1:
        return "head"
    return ("dW_0" if name[0] == "W" else "db_l") if l == 0 else ("dW_l" if name[0] == "W" else "db_l")


def torch_grads(net, pts, U, V, dtype, device="cpu"):
    """{name: float64 CPU gradient} of sum(U f) + sum(V . grad_x f) by torch autograd (V None: of sum(U f))"""
    m = copy.deepcopy(net).to(dtype).to(device)
    p = pts.detach().clone().to(dtype).to(device).requires_grad_(True)
    f = m(p).sdf.squeeze(-1)
    loss = (U.to(dtype).to(device) * f).sum()
    if V is not None:
        g = torch.autograd.grad(f.sum(), p, create_graph=True)[0]
        loss = loss + (V.to(dtype).to(device) * g).sum()
    loss.backward()
    out = {}
    for l, lin in enumerate(m.lins):
        out["W%d" % l] = lin.weight.grad.detach().double().cpu()
        out["b%d" % l] = lin.bias.grad.detach().double().cpu()
    out["points"] = p.grad.detach().double().cpu()
    return out


def tangent_form_grads(net, pts, U, V):
    """The same gradients by the formulas the kernels implement, in the dtype of `net`, without autograd"""
    with torch.no_grad():
        lins = list(net.lins)
        L = len(lins) - 2
        x = pts.to(lins[0].weight.dtype)
        u = U.to(x.dtype)
        v = None if V is None else V.to(x.dtype)
        om = [net.first_omega_0] + [net.hidden_omega_0] * L
        hs, hts, ss, zts = [], [], [], []
        h, ht = x, v
        for l in range(L + 1):
            W, b = lins[l].weight, lins[l].bias
            z = h @ W.t() + b
            s = om[l] * torch.cos(om[l] * z)
            h = torch.sin(om[l] * z)
            hs.append(h); ss.append(s)
            if v is not None:
                zt = ht @ W.t()
                ht = s * zt
                zts.append(zt); hts.append(ht)
        wL = lins[-1].weight.reshape(-1)
        out = {}
        out["W%d" % (L + 1)] = ((u[:, None] * hs[-1]).sum(0) + (hts[-1].sum(0) if v is not None else 0)).reshape(1, -1)
        out["b%d" % (L + 1)] = u.sum().reshape(1)
        hbar = u[:, None] * wL[None, :]
        htbar = wL[None, :].expand_as(hbar)
        for l in range(L, -1, -1):
            zbar = hbar * ss[l]
            if v is not None:
                ztbar = htbar * ss[l]
                zbar = zbar - om[l] ** 2 * hs[l] * zts[l] * htbar
            h_in = x if l == 0 else hs[l - 1]
            out["W%d" % l] = zbar.t() @ h_in
            if v is not None:
                out["W%d" % l] = out["W%d" % l] + ztbar.t() @ (v if l == 0 else hts[l - 1])
            out["b%d" % l] = zbar.sum(0)
            W = lins[l].weight
            hbar = zbar @ W
            if v is not None:
                htbar = ztbar @ W
        out["points"] = hbar
        return {k: t.double() for k, t in out.items()}


def err(g, g64):
    top = g64.abs().max().item()
    d = (g.double() - g64).abs().max().item()
    return d / top if top > 0 else d


def assert_criterion(got, refs, what, n_hidden, keys=None):
    """got: {name: tensor}; refs = (g64, g32_cpu, g32_gpu).  Every figure is printed before anything is asserted."""
    g64, g32c, g32g = refs
    keys = list(keys if keys is not None else sorted(got))
    rows = []
    for k in keys:
        assert got[k].shape == g64[k].shape, (what, k, got[k].shape, g64[k].shape)
        e_hip, e_cpu, e_gpu = err(got[k], g64[k]), err(g32c[k], g64[k]), err(g32g[k], g64[k])
        limit = FACTOR * max(e_cpu, e_gpu) + FLOOR
        cls = class_of(k, n_hidden)
        WORST[cls] = max(WORST.get(cls, 0.0), e_hip / limit)
        print("%s %s [%s]: e_cpu %.3g e_gpu %.3g e_hip %.3g ratio %.3f" % (what, k, cls, e_cpu, e_gpu, e_hip, e_hip / limit))
        rows.append((k, e_cpu, e_gpu, e_hip, limit))
    for k, e_cpu, e_gpu, e_hip, limit in rows:
        assert torch.isfinite(got[k]).all(), "%s %s: non-finite gradient" % (what, k)
        assert e_hip <= limit, (what, k, e_cpu, e_gpu, e_hip)


def references(net, pts, U, V, dev):
    return (torch_grads(net, pts, U, V, torch.float64), torch_grads(net, pts, U, V, torch.float32),
            torch_grads(net, pts, U, V, torch.float32, dev))


def guarded(t):
    """t as a slice out of a larger NaN-filled buffer (contiguous, same values)"""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 512,), float("nan"), dtype=t.dtype)
    buf[256:256 + flat.numel()] = flat
    return buf


def on_gpu(t, dev):
    if t is None:
        return None
    return guarded(t).to(dev)[256:256 + t.numel()].view(t.shape)


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def kernel_width(hidden):
    return next(h for h in (64, 128, 256) if h >= hidden)


def padded_raw(net):
    """The network's weights as the kernels' raw vector at the kernel width (zero rows and columns added), on the CPU"""
    lins = list(net.lins)
    H = kernel_width(lins[0].out_features)
    parts = []
    for i, lin in enumerate(lins):
        w, b = lin.weight.detach().float(), lin.bias.detach().float()
        rows = H if i < len(lins) - 1 else 1
        cols = H if i > 0 else 3
        wp, bp = torch.zeros(rows, cols), torch.zeros(rows)
        wp[:w.shape[0], :w.shape[1]] = w
        bp[:b.shape[0]] = b
        parts += [wp.reshape(-1), bp]
    return torch.cat(parts).contiguous(), H


def abi_grads(net, pts, U, V, dev, want_raw=True, want_pts=True):
    """iso_sirengrad_backward called directly: every input a slice of a NaN-filled buffer, every output and the workspace
    pre-filled with NaN.  Returns {W0.., b0.., points} on the CPU at the MODEL's width; the padded rows and columns are
    checked to be zero."""
    from iso_points_amd import _lib
    lib = _lib.load()
    lins = list(net.lins)
    Hm, L = lins[0].out_features, len(lins) - 2
    raw_cpu, H = padded_raw(net)
    assert lib.iso_sirengrad_form(Hm, L) == 800 + H // 16
    assert raw_cpu.numel() == lib.iso_siren_raw_floats(H, L)
    n = pts.shape[0]
    raw = on_gpu(raw_cpu, dev)
    packed = nan_like((lib.iso_siren_packed_floats(H, L),), dev)
    _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, L, _lib.stream())
    d_pts, d_u, d_v = on_gpu(pts.float(), dev), on_gpu(U.float(), dev), on_gpu(None if V is None else V.float(), dev)
    g_raw = nan_like((raw.numel(),), dev) if want_raw else None
    g_pts = nan_like((n, 3), dev) if want_pts else None
    ws = nan_like((lib.iso_sirengrad_workspace_bytes(n, H, L) // 4,), dev)
    _lib.call("iso_sirengrad_backward", _lib.ptr(d_pts), _lib.ptr(d_u), _lib.ptr(d_v), n, _lib.ptr(raw), _lib.ptr(packed), H, L,
              float(net.first_omega_0), float(net.hidden_omega_0), _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(ws),
              ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    out = {}
    if want_raw:
        g, at = g_raw.cpu(), 0
        assert torch.isfinite(g).all()
        for i in range(L + 2):
            rows, cols = (H if i < L + 1 else 1), (H if i > 0 else 3)
            W = g[at:at + rows * cols].reshape(rows, cols)
            at += rows * cols
            b = g[at:at + rows]
            at += rows
            r, c = (Hm if i < L + 1 else 1), (Hm if i > 0 else 3)
            assert (W[r:] == 0).all() and (W[:, c:] == 0).all() and (b[r:] == 0).all(), ("padding", i)
            out["W%d" % i], out["b%d" % i] = W[:r, :c].contiguous(), b[:r].contiguous()
        assert at == g.numel()
    if want_pts:
        out["points"] = g_pts.cpu()
    return out
