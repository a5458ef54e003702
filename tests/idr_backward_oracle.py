"""Shared by the IDR-backward tests: the float64 oracle (torch autograd of the network of oracle.iso_oracle.IdrSDF on its
EFFECTIVE weights W_l = g v / |v|, on the CPU: autograd.grad(create_graph=True) for g = grad_x f, then the backward of
sum(U f) + sum(V . g) with seeded U, V), the tangent-form formulas of DESIGN.md 3.1d restated in torch without autograd, the
float32 comparison runs and the criterion, which is tests/siren_backward_oracle.py's: per gradient tensor
e = max|grad - grad64| / max|grad64|, e_hip <= 1.5 max(e_cpu, e_gpu) + 2e-7.  No point is filtered out.

Gradient names: W0, b0 .. W{n-1}, b{n-1} (softplus layers), W{n}, b{n} (the head), points."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.iso_oracle import IdrSDF
from siren_backward_oracle import FACTOR, FLOOR, err, nan_like, on_gpu

BETA = 100.0
WORST = {}          # tensor class -> worst e_hip / limit seen by assert_criterion in this process


def make_net(hidden, n_layers, skip, n_freq, seed):
    """IdrSDF with every parameter moved by 0.01 randn: the geometric initialisation zeroes the encoding columns of W_0 and
    of the skip layer, and a wrong encoding path would hide behind them"""
    with torch.random.fork_rng():
        torch.manual_seed(6000 + seed)
        m = IdrSDF(hidden_size=hidden, n_layers=n_layers, skip_in=(skip,) if skip is not None and skip >= 0 else (),
                   num_frequencies=n_freq)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01 * torch.randn_like(p))
    return m


def shape_of(net):
    """(H, n_layers, skip or -1, F)"""
    return net.hidden_size, net.n_layers, (net.skip_in[0] if net.skip_in else -1), net.F


def make_points(n, seed, scale=1.0):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(1000 + seed)) * 2 - 1) * scale


def seeded_UV(n, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn(n, generator=g), torch.randn(n, 3, generator=g)


def effective(net, dtype=torch.float32, device="cpu"):
    """the effective weights and the biases, detached: ([W_0 .. W_n], [b_0 .. b_n])"""
    n_lin = net.num_layers - 1
    return ([net.weight(l).detach().to(dtype).to(device) for l in range(n_lin)],
            [net.b[l].detach().to(dtype).to(device) for l in range(n_lin)])


def embed(x, n_freq):
    outs = [x]
    for k in range(n_freq):
        outs += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(outs, -1)


def forward_eff(Ws, bs, x, n_freq, skip):
    """IdrSDF.forward on explicit effective weights: f (N,)"""
    e = embed(x, n_freq)
    h = e
    for l in range(len(Ws)):
        if l == skip:
            h = torch.cat([h, e], -1) / np.sqrt(2)
        h = F.linear(h, Ws[l], bs[l])
        if l < len(Ws) - 1:
            h = F.softplus(h, beta=BETA)
    return torch.tanh(h).squeeze(-1)


def class_of(name, n_layers):
    if name == "points":
        return "dx"
    l = int(name[1:])
    if l == n_layers:
        return "head"
    return ("dW_0" if l == 0 else "dW_l") if name[0] == "W" else "db_l"


def torch_grads(net, pts, U, V, dtype, device="cpu"):
    """{name: float64 CPU gradient} of sum(U f) + sum(V . grad_x f) by torch autograd (V None: of sum(U f))"""
    H, nl, skip, nf = shape_of(net)
    Ws, bs = effective(net, dtype, device)
    for t in Ws + bs:
        t.requires_grad_(True)
    p = pts.detach().clone().to(dtype).to(device).requires_grad_(True)
    f = forward_eff(Ws, bs, p, nf, skip)
    loss = (U.to(dtype).to(device) * f).sum()
    if V is not None:
        g = torch.autograd.grad(f.sum(), p, create_graph=True)[0]
        loss = loss + (V.to(dtype).to(device) * g).sum()
    loss.backward()
    out = {}
    for l in range(nl + 1):
        out["W%d" % l] = Ws[l].grad.detach().double().cpu()
        out["b%d" % l] = bs[l].grad.detach().double().cpu()
    out["points"] = p.grad.detach().double().cpu()
    return out


def encoding(x, n_freq):
    """e, dval, d2val (N, D0) and coord (D0,) of posenc"""
    e, d1, d2, coord = [x], [torch.ones_like(x)], [torch.zeros_like(x)], [0, 1, 2]
    for k in range(n_freq):
        fr = 2.0 ** k
        s, c = torch.sin(x * fr), torch.cos(x * fr)
        e += [s, c]
        d1 += [fr * c, -fr * s]
        d2 += [-fr * fr * s, -fr * fr * c]
        coord += [0, 1, 2, 0, 1, 2]
    return torch.cat(e, -1), torch.cat(d1, -1), torch.cat(d2, -1), torch.tensor(coord)


def tangent_form_grads(net, pts, U, V, dtype=torch.float64):
    """The same gradients by the formulas the kernels implement, without autograd"""
    with torch.no_grad():
        H, n, skip, nf = shape_of(net)
        Ws, bs = effective(net, dtype)
        x, u = pts.to(dtype), U.to(dtype)
        v = None if V is None else V.to(dtype)
        r2 = np.sqrt(2)
        e, dval, d2val, coord = encoding(x, nf)
        D0 = e.shape[1]
        et = None if v is None else dval * v[:, coord]
        ins, ints, ss, sps, zts = [], [], [], [], []
        h, ht = e, et
        for l in range(n):
            if l == skip:
                h = torch.cat([h, e], -1) / r2
                ht = None if v is None else torch.cat([ht, et], -1) / r2
            ins.append(h); ints.append(ht)
            z = h @ Ws[l].t() + bs[l]
            t = BETA * z
            lin = t > 20
            s = torch.where(lin, torch.ones_like(t), torch.sigmoid(t))
            ss.append(s)
            sps.append(torch.where(lin, torch.zeros_like(t), BETA * s * (1 - s)))
            h = torch.where(lin, z, F.softplus(z, beta=BETA))
            if v is not None:
                zt = ht @ Ws[l].t()
                zts.append(zt)
                ht = s * zt
        wn = Ws[n].reshape(-1)
        f = torch.tanh(h @ wn + bs[n])
        d = 1 - f * f
        yt = 0 if v is None else ht @ wn
        ybar, ytbar = d * (u - 2 * f * yt), d
        out = {}
        dwn = (ybar[:, None] * h).sum(0)
        if v is not None:
            dwn = dwn + (ytbar[:, None] * ht).sum(0)
        out["W%d" % n], out["b%d" % n] = dwn.reshape(1, -1), ybar.sum().reshape(1)
        hbar = ybar[:, None] * wn[None, :]
        htbar = ytbar[:, None] * wn[None, :]
        ebar, etbar = torch.zeros_like(e), torch.zeros_like(e)
        for l in range(n - 1, -1, -1):
            zbar = hbar * ss[l]
            if v is not None:
                ztbar = htbar * ss[l]
                zbar = zbar + htbar * zts[l] * sps[l]
            out["W%d" % l] = zbar.t() @ ins[l]
            if v is not None:
                out["W%d" % l] = out["W%d" % l] + ztbar.t() @ ints[l]
            out["b%d" % l] = zbar.sum(0)
            inbar = zbar @ Ws[l]
            intbar = ztbar @ Ws[l] if v is not None else None
            if l == skip:
                inbar = inbar / r2
                ebar = ebar + inbar[:, H - D0:]
                hbar = inbar[:, :H - D0]
                if v is not None:
                    intbar = intbar / r2
                    etbar = etbar + intbar[:, H - D0:]
                    htbar = intbar[:, :H - D0]
            elif l == 0:
                ebar = ebar + inbar
                if v is not None:
                    etbar = etbar + intbar
            else:
                hbar, htbar = inbar, intbar
        per = ebar * dval
        if v is not None:
            per = per + etbar * d2val * v[:, coord]
        dx = torch.zeros_like(x)
        dx.index_add_(1, coord, per)
        out["points"] = dx
        return {k: t.double() for k, t in out.items()}


def assert_criterion(got, refs, what, n_layers, keys=None):
    """got: {name: tensor}; refs = (g64, g32_cpu, g32_gpu).  Every figure is printed before anything is asserted."""
    g64, g32c, g32g = refs
    keys = list(keys if keys is not None else sorted(got))
    rows = []
    for k in keys:
        assert got[k].shape == g64[k].shape, (what, k, got[k].shape, g64[k].shape)
        e_hip, e_cpu, e_gpu = err(got[k], g64[k]), err(g32c[k], g64[k]), err(g32g[k], g64[k])
        limit = FACTOR * max(e_cpu, e_gpu) + FLOOR
        cls = class_of(k, n_layers)
        WORST[cls] = max(WORST.get(cls, 0.0), e_hip / limit)
        print("%s %s [%s]: e_cpu %.3g e_gpu %.3g e_hip %.3g ratio %.3f" % (what, k, cls, e_cpu, e_gpu, e_hip, e_hip / limit))
        rows.append((k, e_cpu, e_gpu, e_hip, limit))
    for k, e_cpu, e_gpu, e_hip, limit in rows:
        assert torch.isfinite(got[k]).all(), "%s %s: non-finite gradient" % (what, k)
        assert e_hip <= limit, (what, k, e_cpu, e_gpu, e_hip)


def references(net, pts, U, V, dev):
    return (torch_grads(net, pts, U, V, torch.float64), torch_grads(net, pts, U, V, torch.float32),
            torch_grads(net, pts, U, V, torch.float32, dev))


def raw_of(net):
    Ws, bs = effective(net)
    return torch.cat([t.reshape(-1) for W, b in zip(Ws, bs) for t in (W, b)]).contiguous()


def abi_grads(net, pts, U, V, dev, want_raw=True, want_pts=True):
    """iso_idrgrad_backward called directly: every input a slice of a NaN-filled buffer, every output and the workspace
    pre-filled with NaN.  Returns {W0.., b0.., points} on the CPU.  The narrow layer's padded rows -- columns H - D0 .. H of
    its derivative stash, which the header's workspace layout places -- are checked to hold exactly zero adjoints."""
    from iso_points_amd import _lib
    lib = _lib.load()
    H, nl, skip, nf = shape_of(net)
    D0 = 3 + 6 * nf
    assert lib.iso_idrgrad_form(H, nl, skip, nf) == 900 + H // 16
    raw_cpu = raw_of(net)
    assert raw_cpu.numel() == lib.iso_idr_raw_floats(H, nl, skip, nf)
    n = pts.shape[0]
    raw = on_gpu(raw_cpu, dev)
    packed = nan_like((lib.iso_idr_packed_floats(H, nl),), dev)
    _lib.call("iso_idr_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, nl, skip, nf, _lib.stream())
    d_pts, d_u, d_v = on_gpu(pts.float(), dev), on_gpu(U.float(), dev), on_gpu(None if V is None else V.float(), dev)
    g_raw = nan_like((raw.numel(),), dev) if want_raw else None
    g_pts = nan_like((n, 3), dev) if want_pts else None
    ws = nan_like((lib.iso_idrgrad_workspace_bytes(n, H, nl, skip, nf) // 4,), dev)
    _lib.call("iso_idrgrad_backward", _lib.ptr(d_pts), _lib.ptr(d_u), _lib.ptr(d_v), n, _lib.ptr(raw), _lib.ptr(packed), H, nl,
              skip, nf, BETA, _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(ws), ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    if skip >= 1 and n > 0:
        wsp = lib.iso_idrgrad_workspace_points()
        mw = min(n, wsp)
        rows = (2 if V is not None else 1) * (n - (n - 1) // wsp * wsp)          # the last workspace chunk's
        sst = 512 + 2 * mw * 64 + nl * 2 * mw * H
        slot = ws[sst + (skip - 1) * 2 * mw * H:][:rows * H].reshape(rows, H)
        assert (slot[:, H - D0:] == 0).all(), "adjoints in the narrow layer's padded rows"
        assert torch.isfinite(slot).all()
    out = {}
    if want_raw:
        g, at = g_raw.cpu(), 0
        assert torch.isfinite(g).all()
        for l in range(nl + 1):
            rows = 1 if l == nl else (H - D0 if (skip >= 1 and l == skip - 1) else H)
            cols = D0 if l == 0 else H
            out["W%d" % l] = g[at:at + rows * cols].reshape(rows, cols).clone()
            at += rows * cols
            out["b%d" % l] = g[at:at + rows].clone()
            at += rows
        assert at == g.numel()
    if want_pts:
        out["points"] = g_pts.cpu()
    return out
