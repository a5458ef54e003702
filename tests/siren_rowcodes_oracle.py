"""Shared by the tests of the SIREN backward with one latent code per cloud (iso_sirencode_backward; siren_forward's
cloud_idx= / lengths=).  The oracle is torch autograd in float64 on the CPU of the same network with the TABLE of layer-0
biases as a leaf: z_0 = x W0x^T + table[code_of], g by autograd.grad(create_graph=True), loss sum(U f) + sum(V . g) with
seeded U, V; the float32 runs of the same on the CPU and eagerly on the GPU are the comparison.  The criterion is
tests/siren_backward_oracle.py's (assert_criterion); the table's gradient dt counts as class db_l and is handed to it under
the name b0 of a call of its own.

Gradient names: W0 (the xyz columns' dW0x), b0 (the sum of zbar_0 over ALL points = sum_u dt_u), W1.. / b1.., the head,
points, dt (U, H)."""
import copy

import torch

from siren_backward_oracle import assert_criterion, kernel_width, nan_like, on_gpu, padded_raw, references  # noqa: F401

WORST_CODE = {}     # "d codes" etc. through torch's chain: worst e_hip / limit seen by assert_rule_named


def make_table(net, n_codes, seed, tail=True):
    """(table (U, Hm) f32, tail (U, Hm) f32 or None): rows around the network's own b_0, and what a rounding would have lost"""
    g = torch.Generator().manual_seed(7000 + seed)
    b0 = net.lins[0].bias.detach().float()
    table = (b0[None, :] + 0.1 * torch.randn(n_codes, b0.numel(), generator=g)).contiguous()
    t = (table.abs() * 2.0 ** -25 * (torch.rand(table.shape, generator=g) * 2 - 1)).contiguous() if tail else None
    return table, t


def rows_from_lengths(lengths):
    """(code_of (n,) int32, code_first (U + 1,) int64)"""
    code_of = torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int32), torch.tensor(lengths, dtype=torch.int64))
    first = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    first[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
    return code_of, first


def table_forward(m, p, t, idx):
    lins = list(m.lins)
    h = torch.sin(m.first_omega_0 * (p @ lins[0].weight.t() + t[idx]))
    for lin in lins[1:-1]:
        h = torch.sin(m.hidden_omega_0 * lin(h))
    return lins[-1](h).squeeze(-1)


def table_grads(net, table, tail, code_of, pts, U, V, dtype, device="cpu"):
    """{name: float64 CPU gradient} of sum(U f) + sum(V . grad_x f) (V None: of sum(U f)) with the table as a leaf; the
    float64 run adds the tail to the table, the float32 runs have no use for it"""
    m = copy.deepcopy(net).to(dtype).to(device)
    p = pts.detach().clone().to(dtype).to(device).requires_grad_(True)
    t = table.detach().clone().to(dtype)
    if tail is not None and dtype == torch.float64:
        t = t + tail.double()
    t = t.to(device).requires_grad_(True)
    idx = code_of.long().to(device)
    f = table_forward(m, p, t, idx)
    loss = (U.to(dtype).to(device) * f).sum()
    if V is not None:
        g = torch.autograd.grad(f.sum(), p, create_graph=True)[0]
        loss = loss + (V.to(dtype).to(device) * g).sum()
    loss.backward()
    out = {}
    for l, lin in enumerate(m.lins):
        out["W%d" % l] = lin.weight.grad.detach().double().cpu()
        if l > 0:
            out["b%d" % l] = lin.bias.grad.detach().double().cpu()
    out["dt"] = t.grad.detach().double().cpu()
    out["b0"] = out["dt"].sum(0)
    out["points"] = p.grad.detach().double().cpu()
    return out


def table_references(net, table, tail, code_of, pts, U, V, dev):
    return (table_grads(net, table, tail, code_of, pts, U, V, torch.float64),
            table_grads(net, table, tail, code_of, pts, U, V, torch.float32),
            table_grads(net, table, tail, code_of, pts, U, V, torch.float32, dev))


def table_form_grads(net, table, code_of, pts, U, V):
    """The same gradients by the formulas of the issue's "The mathematics" (DESIGN.md 3.1c), in the dtype of `net`, without
    autograd: siren_backward_oracle.tangent_form_grads with z_0 = W0x x + t_u(p), plus dt_u = sum_{p in u} zbar_0(p)"""
    with torch.no_grad():
        lins = list(net.lins)
        L = len(lins) - 2
        x = pts.to(lins[0].weight.dtype)
        u = U.to(x.dtype)
        v = None if V is None else V.to(x.dtype)
        idx = code_of.long()
        om = [net.first_omega_0] + [net.hidden_omega_0] * L
        hs, hts, ss, zts = [], [], [], []
        h, ht = x, v
        for l in range(L + 1):
            W = lins[l].weight
            z = h @ W.t() + (table.to(x.dtype)[idx] if l == 0 else lins[l].bias)
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
            if l == 0:
                out["dt"] = torch.zeros_like(table, dtype=x.dtype).index_add_(0, idx, zbar)
            W = lins[l].weight
            hbar = zbar @ W
            if v is not None:
                htbar = ztbar @ W
        out["points"] = hbar
        return {k: t.double() for k, t in out.items()}


def assert_table_criterion(got, refs, what, n_hidden):
    """assert_criterion on every gradient; dt as class db_l (under the name b0, in a call of its own)"""
    rest = [k for k in sorted(got) if k != "dt"]
    if "dt" in got:
        assert_criterion({"b0": got["dt"]}, tuple({"b0": r["dt"]} for r in refs), (what, "dt as db_l"), n_hidden)
    assert_criterion({k: got[k] for k in rest}, refs, what, n_hidden, keys=rest)


def coded_abi_grads(net, table, tail, lengths, pts, U, V, dev, want_raw=True, want_tab=True, want_pts=True, rows=None):
    """iso_sirencode_backward called directly: every input a slice of a NaN-filled buffer, every output and the workspace
    pre-filled with NaN.  Returns {W0.., b0.., points, dt} on the CPU at the MODEL's width; the padded rows and columns are
    checked to be zero.  rows: (code_of, code_first) in place of those of `lengths`."""
    from iso_points_amd import _lib
    lib = _lib.load()
    lins = list(net.lins)
    Hm, L = lins[0].out_features, len(lins) - 2
    raw_cpu, H = padded_raw(net)
    raw_cpu[3 * H:4 * H] = float("nan")                   # b_0 of the image is not read: the table holds it
    n, n_codes = pts.shape[0], table.shape[0]
    code_of, code_first = rows if rows is not None else rows_from_lengths(lengths)
    assert code_of.numel() == n

    def pad(t):
        if t is None:
            return None
        out = torch.zeros(n_codes, H)
        out[:, :Hm] = t
        return out
    raw = on_gpu(raw_cpu, dev)
    packed = nan_like((lib.iso_siren_packed_floats(H, L),), dev)
    _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, L, _lib.stream())
    d_pts, d_u, d_v = on_gpu(pts.float(), dev), on_gpu(U.float(), dev), on_gpu(None if V is None else V.float(), dev)
    d_tab, d_tail = on_gpu(pad(table), dev), on_gpu(pad(tail), dev)
    d_of, d_first = on_gpu_int(code_of, dev), on_gpu_int(code_first, dev)
    g_raw = nan_like((raw.numel(),), dev) if want_raw else None
    g_tab = nan_like((n_codes, H), dev) if want_tab else None
    g_pts = nan_like((n, 3), dev) if want_pts else None
    ws = nan_like((lib.iso_sirencode_workspace_bytes(n, H, L, n_codes) // 4,), dev)
    _lib.call("iso_sirencode_backward", _lib.ptr(d_pts), _lib.ptr(d_u), _lib.ptr(d_v), n, _lib.ptr(packed), H, L,
              float(net.first_omega_0), float(net.hidden_omega_0), _lib.ptr(d_tab), _lib.ptr(d_tail), _lib.ptr(d_of),
              _lib.ptr(d_first), n_codes, _lib.ptr(g_raw), _lib.ptr(g_tab), _lib.ptr(g_pts), _lib.ptr(ws), ws.numel() * 4,
              _lib.stream())
    torch.cuda.synchronize()
    out = {}
    if want_raw:
        g, at = g_raw.cpu(), 0
        assert torch.isfinite(g).all()
        for i in range(L + 2):
            rws, cols = (H if i < L + 1 else 1), (H if i > 0 else 3)
            W = g[at:at + rws * cols].reshape(rws, cols)
            at += rws * cols
            b = g[at:at + rws]
            at += rws
            r, c = (Hm if i < L + 1 else 1), (Hm if i > 0 else 3)
            assert (W[r:] == 0).all() and (W[:, c:] == 0).all() and (b[r:] == 0).all(), ("padding", i)
            out["W%d" % i], out["b%d" % i] = W[:r, :c].contiguous(), b[:r].contiguous()
        assert at == g.numel()
    if want_tab:
        g = g_tab.cpu()
        assert torch.isfinite(g).all() and (g[:, Hm:] == 0).all(), "padded columns of dt"
        out["dt"] = g[:, :Hm].contiguous()
    if want_pts:
        out["points"] = g_pts.cpu()
    return out


def on_gpu_int(t, dev):
    """an integer tensor as a 16-byte aligned slice of a buffer filled with an index far out of range"""
    buf = torch.full((t.numel() + 32,), 2 ** 30 if t.dtype == torch.int32 else 2 ** 40, dtype=t.dtype)
    buf[16:16 + t.numel()] = t
    return buf.to(dev)[16:16 + t.numel()]
