"""SDF network definitions the fused projection kernels understand, and the weight
extraction that feeds them.

`Siren` / `SineLayer` mirror the *forward definition* of the reference's classes
(DSS/models/common.py:56-165: same constructor arguments, same attribute layout
`net[i].linear.{weight,bias}` / `omega_0`, same initialisation) so that a model built
by the reference's config factory and one built here are interchangeable for
`UniformProjection`.  Weights are re-read on every call (they change every optimiser
step).
"""
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib

_fields = ("sdf", "latent", "rgb", "occupancy")
NetOutput = namedtuple("Result", _fields, defaults=(None,) * len(_fields))
# the codes of one call of a latent-conditioned SIREN as the kernels take them (code_rows): codes (U, C) f32 and the
# table row of every point, code_of (n,) int32 -- None when U = 1 (one code for every point)
CodeRows = namedtuple("CodeRows", ("codes", "code_of"))


class SphereSDF(nn.Module):
    """Analytic |x-c|-R (BASELINE.json configs[0]); `iso_analytic` routes it to
    iso_project_sphere."""
    iso_analytic = "sphere"

    def __init__(self, center=(0.0, 0.0, 0.0), radius=1.0):
        super().__init__()
        self.register_buffer("center", torch.tensor(center, dtype=torch.float32))
        self.radius = float(radius)

    def forward(self, x, **kwargs):
        return NetOutput(sdf=(x - self.center).norm(dim=-1, keepdim=True) - self.radius)


class SineLayer(nn.Module):
    """common.py:56-87."""

    def __init__(self, dim, out_dim, bias=True, is_first=False, omega_0=30):
        super().__init__()
        self.omega_0 = omega_0
        self.is_first = is_first
        self.dim = dim
        self.linear = nn.Linear(dim, out_dim, bias=bias)
        with torch.no_grad():
            if is_first:
                self.linear.weight.uniform_(-1 / dim, 1 / dim)
            else:
                b = np.sqrt(6 / dim) / omega_0
                self.linear.weight.uniform_(-b, b)

    def forward(self, input):
        return torch.sin(self.omega_0 * self.linear(input))


class Siren(nn.Module):
    """common.py:90-165 restricted to what the hot path uses: sdf output, linear head.  c_dim > 0 (the reference's
    default, config.py:163-166) conditions it on a latent code: the first sine layer is dim + c_dim wide and forward
    concatenates [c, coords] (:150-152); the fused kernels fold the code into layer 0's bias (PackedSiren.fold)."""

    def __init__(self, dim=3, hidden_size=256, n_layers=3, out_dims=None, outermost_linear=True,
                 c_dim=0, first_omega_0=30, hidden_omega_0=30.0, activation=None, **kwargs):
        super().__init__()
        out_dims = out_dims or OrderedDict(sdf=1)
        if c_dim < 0 or not outermost_linear or activation is not None or sum(out_dims.values()) != 1:
            raise NotImplementedError("iso_points_amd.Siren covers the sdf-only, linear-head "
                                      "configuration of the reference's Siren")
        self.dim, self.c_dim = dim, c_dim
        net = [SineLayer(dim + c_dim, hidden_size, is_first=True, omega_0=first_omega_0)]
        for _ in range(n_layers):
            net.append(SineLayer(hidden_size, hidden_size, is_first=False, omega_0=hidden_omega_0))
        final = nn.Linear(hidden_size, 1)
        with torch.no_grad():
            b = np.sqrt(6 / hidden_size) / hidden_omega_0
            final.weight.uniform_(-b, b)
        net.append(final)
        self.net = nn.Sequential(*net)

    def forward(self, coords, c=None, **kwargs):
        if c is not None and c.numel() > 0:                 # common.py:150-152
            assert coords.ndim == c.ndim
            coords = torch.cat([c, coords], dim=-1)
        return NetOutput(sdf=self.net(coords))


def coded_siren_spec(model):
    """(lins, omega_first, omega_hidden, c_dim) if `model` is a latent-conditioned SIREN the fused kernels can run (the
    reference's Siren(c_dim = C > 0) or ours: `.net[i].linear`, layer 0 (3 + C) wide with the code columns FIRST, as
    forward concatenates [c, x]), else None.  lins[0].weight[:, :c_dim] are the code columns, [:, c_dim:] the xyz
    columns.  siren_spec() stays None for these models: only the callers that pass a code take them."""
    C = getattr(model, "c_dim", 0)
    if not isinstance(C, int) or C <= 0 or not (hasattr(model, "net") and isinstance(model.net, nn.Sequential)):
        return None
    mods = list(model.net)
    if len(mods) < 2 or not isinstance(mods[-1], nn.Linear):
        return None
    if not all(hasattr(m, "linear") and hasattr(m, "omega_0") for m in mods[:-1]):
        return None
    lins = [m.linear for m in mods[:-1]] + [mods[-1]]
    omegas = [float(m.omega_0) for m in mods[:-1]]
    if lins[0].in_features != 3 + C or not _siren_shape_ok(lins, omegas):
        return None
    return lins, omegas[0], (omegas[1] if len(omegas) > 1 else omegas[0]), C


def code_rows(c, c_dim, counts):
    """The code shapes the reference's callers pass, as the fused kernels take them: (codes (U, c_dim) f32, code_of) or
    None (the generic route).  counts: host list, number of points (rays, pairs) of each batch row, in packed order.
      (C,) / (1, C) / (1, 1, C)  one code for every point: U = 1, code_of None
      (N, C) / (N, 1, C)         one code per row, N = len(counts): code_of (sum(counts),) int32 on c's device, row b
                                 repeated counts[b] times
    Anything else (per-point codes, a row count that is not the batch's) is None."""
    if not torch.is_tensor(c) or c.numel() == 0 or c.shape[-1] != c_dim or c.dtype not in (torch.float32, torch.float64,
                                                                                          torch.float16, torch.bfloat16):
        return None
    if c.ndim == 1 or (c.ndim in (2, 3) and all(d == 1 for d in c.shape[:-1])):
        return CodeRows(c.detach().reshape(1, c_dim).float().contiguous(), None)
    if c.ndim == 3 and c.shape[1] != 1:
        return None
    if c.ndim not in (2, 3) or c.shape[0] != len(counts):
        return None
    codes = c.detach().reshape(-1, c_dim).float().contiguous()
    return CodeRows(codes, rows_of(counts, c.device))


def rows_of(counts, device):
    """(sum(counts),) int32 on `device`: b repeated counts[b] times (host list in, no host read)"""
    reps = torch.tensor([int(x) for x in counts], dtype=torch.int64, device=device)
    return torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32, device=device), reps,
                                   output_size=int(sum(int(x) for x in counts)))


def _siren_shape_ok(lins, omegas):
    """3 (+ code columns) -> H -> H.. -> 1 with H <= 256, <= 8 hidden layers, biases, one hidden omega"""
    H = lins[0].out_features
    if lins[-1].out_features != 1 or lins[-1].in_features != H:
        return False
    if H < 1 or H > 256 or len(lins) - 2 > 8:
        return False
    if any(lin.in_features != H or lin.out_features != H for lin in lins[1:-1]):
        return False
    if any(lin.bias is None for lin in lins):
        return False
    return len(set(omegas[1:])) <= 1


def siren_spec(model):
    """Return (linears, omega_first, omega_hidden) if `model` is a SIREN the fused kernel
    can run (3 -> H -> H.. -> 1, sine layers with equal hidden omega, linear head), else None.
    Accepts the reference's Siren (`.net`), ours, and the oracle's SirenSDF (`.lins`)."""
    lins, omegas = None, None
    if hasattr(model, "net") and isinstance(model.net, nn.Sequential):
        mods = list(model.net)
        if len(mods) < 2 or not isinstance(mods[-1], nn.Linear):
            return None
        if getattr(model, "c_dim", 0) not in (0, None):
            return None
        if not all(hasattr(m, "linear") and hasattr(m, "omega_0") for m in mods[:-1]):
            return None
        lins = [m.linear for m in mods[:-1]] + [mods[-1]]
        omegas = [float(m.omega_0) for m in mods[:-1]]
    elif hasattr(model, "lins") and hasattr(model, "first_omega_0"):
        lins = list(model.lins)
        omegas = [float(model.first_omega_0)] + [float(model.hidden_omega_0)] * (len(lins) - 2)
    else:
        return None
    H = lins[0].out_features
    if lins[0].in_features != 3 or lins[-1].out_features != 1 or lins[-1].in_features != H:
        return None
    if H < 1 or H > 256 or len(lins) - 2 > 8:       # widths other than 64 / 128 / 256 are zero-padded up (PackedSiren)
        return None
    for lin in lins[1:-1]:
        if lin.in_features != H or lin.out_features != H:
            return None
    if any(lin.bias is None for lin in lins):
        return None
    if len(set(omegas[1:])) > 1:
        return None
    return lins, omegas[0], (omegas[1] if len(omegas) > 1 else omegas[0])


def weights_key(lins, device):
    """Identity of a network's weights as the packed images see them: storage address and in-place version of every
    weight / bias.  An optimiser step (in-place) or a re-assigned .data changes it -- but an in-place update THROUGH
    `.data` (p.data.mul_(), p.data.copy_(): EMA, weight clipping, hand-written optimisers) or a raw-pointer write bumps
    neither, so this key is only a sanity check inside one operator call (UniformProjection._packing); across calls a
    weight image is re-used on the caller's explicit word only (reuse_packed)."""
    return (str(device),) + tuple((t.data_ptr(), t._version) for lin in lins for t in (lin.weight, lin.bias))


class PackedSiren(object):
    """Device-side MFMA weight image of a SIREN (iso_siren_pack_weights).  `key` = weights_key at packing time;
    `current(model)` is necessary, not sufficient, for the image to be up to date (see weights_key)."""

    def current(self, model, device):
        spec = siren_spec(model) or coded_siren_spec(model)
        return spec is not None and weights_key(spec[0], device) == self.key

    def __init__(self, model, device):
        spec = siren_spec(model)
        coded = coded_siren_spec(model) if spec is None else None
        if spec is None and coded is None:
            raise ValueError("model is not a SIREN the fused kernel supports")
        # a latent-conditioned SIREN (coded_siren_spec) is packed as the network of its xyz columns W0[:, C:]; the code
        # columns and b0 stay on the device for fold(), which turns the codes of a call into layer 0's biases
        self.c_dim = coded[3] if coded is not None else 0
        lins, self.omega_first, self.omega_hidden = spec if spec is not None else coded[:3]
        self.key = weights_key(lins, device)
        self.model_hidden = lins[0].out_features
        # the fused kernels exist for H = 64 / 128 / 256: any other width runs as the next one up with ZERO rows and
        # columns added -- a padded unit has z = 0, sin(0) = 0 and feeds zero columns, so value and gradient are those
        # of the unpadded network (zeros add exactly nothing to a sum)
        self.hidden = H = next(h for h in (64, 128, 256) if h >= self.model_hidden)
        self.n_hidden = len(lins) - 2
        parts = []
        for i, lin in enumerate(lins):
            w = lin.weight.detach().to(device=device, dtype=torch.float32)
            b = lin.bias.detach().to(device=device, dtype=torch.float32)
            if i == 0 and self.c_dim:
                self.w0_code = w[:, :self.c_dim].contiguous()            # (H_model, C)
                self.b0 = b.contiguous()                                  # (H_model,)
                w = w[:, self.c_dim:]
            rows = H if i < len(lins) - 1 else w.shape[0]
            cols = H if i > 0 else w.shape[1]
            if (rows, cols) != tuple(w.shape):
                wp = w.new_zeros((rows, cols))
                wp[:w.shape[0], :w.shape[1]] = w
                bp = b.new_zeros((rows,))
                bp[:b.shape[0]] = b
                w, b = wp, bp
            parts += [w.reshape(-1), b.reshape(-1)]
        raw = torch.cat(parts).contiguous()
        lib = _lib.load()
        assert raw.numel() == lib.iso_siren_raw_floats(self.hidden, self.n_hidden)
        self.packed = torch.empty((lib.iso_siren_packed_floats(self.hidden, self.n_hidden),),
                                  dtype=torch.float32, device=device)
        _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(self.packed), self.hidden,
                  self.n_hidden, _lib.stream())
        self._ws = None

    def fold(self, codes):
        """codes (U, c_dim) f32 on the device -> layer 0's bias of every code, (U, hidden) f32 (iso_siren_fold_codes: one
        launch, no host read): b0 + W0[:, :C] c_u in natural feature order, padded features 0.  Separate from the
        weight image, which is re-used across calls while the codes change every call."""
        assert self.c_dim and codes.ndim == 2 and codes.shape[1] == self.c_dim
        codes = codes.detach().to(device=self.packed.device, dtype=torch.float32).contiguous()
        table = torch.empty((codes.shape[0], self.hidden), dtype=torch.float32, device=self.packed.device)
        _lib.call("iso_siren_fold_codes", _lib.ptr(self.w0_code), _lib.ptr(self.b0), _lib.ptr(codes), _lib.ptr(table),
                  self.model_hidden, self.hidden, self.c_dim, codes.shape[0], _lib.stream())
        return table

    def workspace(self, n):
        need = _lib.load().iso_project_siren_workspace_bytes(int(n), self.hidden, self.n_hidden)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=self.packed.device)
        return self._ws


def siren_sdf_and_grad(model, points, need_grad=True, packed=None, code=None):
    """One fused SDF + gradient evaluation (UniformProjection._compute_sdf_and_grad,
    levelset_sampling.py:142-170) for a SIREN.  points (...,3) -> sdf (...), grad (...,3).
    need_grad=False: value only (forward sweep only), grad is None.
    code: CodeRows of a latent-conditioned SIREN (code_rows); required for those, refused for the others."""
    shp = points.shape
    pts = points.detach().reshape(-1, 3).float().contiguous()
    ps = packed if packed is not None else PackedSiren(model, pts.device)
    if bool(ps.c_dim) != (code is not None):
        raise ValueError("a latent-conditioned SIREN needs its code, an unconditioned one takes none")
    n = pts.shape[0]
    sdf = torch.empty((n,), dtype=torch.float32, device=pts.device)
    grad = torch.empty((n, 3), dtype=torch.float32, device=pts.device) if need_grad else None
    ws = ps.workspace(n)
    args = [_lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(grad), n, _lib.ptr(ps.packed), ps.hidden, ps.n_hidden, ps.omega_first,
            ps.omega_hidden, _lib.ptr(ws), ws.numel(), _lib.stream()]
    if code is None:
        _lib.call("iso_siren_sdf_grad", *args)
    else:
        table, code_of = ps.fold(code.codes), code.code_of
        _lib.call("iso_siren_sdf_grad_coded", *args, _lib.ptr(table), _lib.ptr(code_of), table.shape[0])
    return sdf.view(shp[:-1]), (grad.view(shp) if need_grad else None)


# ----------------------------------------------------------------------------- training a SIREN on the fused kernels
def _padded_raw(wb, H, device):
    """The effective W_0, b_0, .., W_L, b_L as the kernels' raw vector at kernel width H (PackedSiren's zero padding)."""
    parts, nl = [], len(wb) // 2
    for i in range(nl):
        w = wb[2 * i].detach().to(device=device, dtype=torch.float32)
        b = wb[2 * i + 1].detach().to(device=device, dtype=torch.float32)
        rows = H if i < nl - 1 else w.shape[0]
        cols = H if i > 0 else w.shape[1]
        if (rows, cols) != tuple(w.shape):
            wp = w.new_zeros((rows, cols))
            wp[:w.shape[0], :w.shape[1]] = w
            bp = b.new_zeros((rows,))
            bp[:b.shape[0]] = b
            w, b = wp, bp
        parts += [w.reshape(-1), b.reshape(-1)]
    return torch.cat(parts).contiguous()


def _pack_raw(raw, H, L):
    lib = _lib.load()
    assert raw.numel() == lib.iso_siren_raw_floats(H, L)
    packed = torch.empty((lib.iso_siren_packed_floats(H, L),), dtype=torch.float32, device=raw.device)
    _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, L, _lib.stream())
    return packed


class _SirenFunction(torch.autograd.Function):
    """sdf (n,) and grad (n, 3) of the fused evaluation (iso_siren_sdf_grad, in whichever GEMM mode the library is in), with
    the fused backward (csrc/sirengrad.hip, iso_sirengrad_backward: the f32-MFMA evaluation of the same network,
    differentiated) into the points and the EFFECTIVE weights and biases W_0, b_0, .., W_L, b_L: those are made under grad
    by the caller, so whatever parametrisation sits above them (a latent code folded into b_0, the xyz columns of a wider
    W_0) gets its gradient from torch's own chain.  Only the inputs are kept; the backward packs the weight image again.
    need_grad False: value only, the second output is an empty, non-differentiable tensor.
    b0_tail (model width,) f32 or None: the bits layer 0's f32 bias lost when it was formed (a latent code folded in float64);
    the backward adds them back in float64 (iso_sirengrad_backward_b0), the forward's values are those of the f32 bias."""

    @staticmethod
    def forward(ctx, shape, need_grad, b0_tail, pts, *wb):
        H, L, w0, wh = shape
        dev, n = pts.device, pts.shape[0]
        lib = _lib.load()
        if not lib.iso_sirengrad_form(H, L):
            raise RuntimeError("iso_points_amd: no fused SIREN backward for hidden %d, %d hidden layers" % (H, L))
        packed = _pack_raw(_padded_raw(wb, H, dev), H, L)
        sdf = torch.empty((n,), dtype=torch.float32, device=dev)
        grad = torch.empty((n, 3) if need_grad else (0, 3), dtype=torch.float32, device=dev)
        ws = torch.empty((lib.iso_project_siren_workspace_bytes(n, H, L),), dtype=torch.uint8, device=dev)
        _lib.call("iso_siren_sdf_grad", _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(grad) if need_grad else None, n,
                  _lib.ptr(packed), H, L, w0, wh, _lib.ptr(ws), ws.numel(), _lib.stream())
        ctx.shape, ctx.need_grad, ctx.b0_tail = shape, need_grad, b0_tail
        ctx.save_for_backward(pts, *wb)
        ctx.set_materialize_grads(False)
        if not need_grad:
            ctx.mark_non_differentiable(grad)
        return sdf, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sdf, g_grad):
        H, L, w0, wh = ctx.shape
        pts, wb = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dev, n = pts.device, pts.shape[0]
        need = ctx.needs_input_grad
        if g_sdf is None and (g_grad is None or not ctx.need_grad):
            return (None,) * len(need)
        lib = _lib.load()
        raw = _padded_raw(wb, H, dev)
        packed = _pack_raw(raw, H, L)
        u = torch.zeros((n,), dtype=torch.float32, device=dev) if g_sdf is None else \
            g_sdf.reshape(n).to(torch.float32).contiguous()
        v = g_grad.reshape(n, 3).to(torch.float32).contiguous() if (ctx.need_grad and g_grad is not None) else None
        g_pts = torch.empty_like(pts) if need[3] else None
        g_raw = torch.empty_like(raw) if any(need[4:]) else None      # NULL: no dW / db work is done
        tail = None
        if ctx.b0_tail is not None:
            tail = torch.zeros((H,), dtype=torch.float32, device=dev)
            tail[:ctx.b0_tail.numel()] = ctx.b0_tail.detach().to(device=dev, dtype=torch.float32)
        ws = torch.empty((lib.iso_sirengrad_workspace_bytes(n, H, L),), dtype=torch.uint8, device=dev)
        args = [_lib.ptr(pts), _lib.ptr(u), _lib.ptr(v), n, _lib.ptr(raw), _lib.ptr(packed), H, L, w0, wh, _lib.ptr(g_raw),
                _lib.ptr(g_pts), _lib.ptr(ws), ws.numel(), _lib.stream()]
        if tail is None:
            _lib.call("iso_sirengrad_backward", *args)
        else:
            _lib.call("iso_sirengrad_backward_b0", *args, _lib.ptr(tail))
        grads, at, nl = [], 0, len(wb) // 2
        for i in range(nl):
            w, b = wb[2 * i], wb[2 * i + 1]
            rows = H if i < nl - 1 else w.shape[0]
            cols = H if i > 0 else w.shape[1]
            grads.append(g_raw[at:at + rows * cols].reshape(rows, cols)[:w.shape[0], :w.shape[1]].to(w.dtype)
                         if need[4 + 2 * i] else None)
            at += rows * cols
            grads.append(g_raw[at:at + rows][:b.shape[0]].to(b.dtype) if need[5 + 2 * i] else None)
            at += rows
        return (None, None, None, g_pts) + tuple(grads)


def cloud_order(cloud_idx, n_codes):
    """The packed order of points given with the row of each: cloud_idx (n,) integers in any order -> (order, inverse,
    code_of, code_first), all on cloud_idx's device and made without a host read.  The indices are clamped into
    [0, n_codes); order (n,) int64 is the stable argsort (points of a row keep their order), inverse its inverse
    (sorted[inverse] is the caller's order), code_of (n,) int32 the sorted rows and code_first (n_codes + 1,) int64 where
    each row starts in the sorted order (searchsorted; a row without points has code_first[u] == code_first[u + 1])."""
    idx = cloud_idx.reshape(-1).to(torch.int64).clamp(0, n_codes - 1)
    order = torch.argsort(idx, stable=True)
    code_of = idx[order]
    code_first = torch.searchsorted(code_of, torch.arange(n_codes + 1, dtype=torch.int64, device=idx.device))
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel(), dtype=torch.int64, device=idx.device)
    return order, inverse, code_of.to(torch.int32), code_first


def _per_cloud_arguments(model, points, c, cloud_idx, lengths):
    """Checks of siren_forward's per-cloud call, before anything is launched: (coded spec, U, n)"""
    if cloud_idx is not None and lengths is not None:
        raise ValueError("iso_points_amd: give cloud_idx or lengths, not both")
    coded = coded_siren_spec(model)
    if coded is None:
        raise ValueError("iso_points_amd: cloud_idx / lengths are for a latent-conditioned SIREN (coded_siren_spec)")
    C = coded[3]
    if not torch.is_tensor(c) or c.ndim != 2 or c.shape[0] < 1 or c.shape[1] != C or not c.is_floating_point():
        raise ValueError("iso_points_amd: with cloud_idx / lengths the codes are c (U, %d), one row per cloud" % C)
    if not torch.is_tensor(points) or points.ndim < 1 or points.shape[-1] != 3:
        raise ValueError("iso_points_amd: points must be (..., 3)")
    U, n = c.shape[0], points.numel() // 3
    if lengths is not None:
        lengths = [int(x) for x in lengths]
        if len(lengths) != U or any(x < 0 for x in lengths) or sum(lengths) != n:
            raise ValueError("iso_points_amd: lengths must be %d counts >= 0 that sum to the %d points" % (U, n))
    else:
        if not torch.is_tensor(cloud_idx) or cloud_idx.is_floating_point() or cloud_idx.is_complex() \
                or cloud_idx.dtype == torch.bool or cloud_idx.numel() != n or cloud_idx.device != points.device:
            raise ValueError("iso_points_amd: cloud_idx must be %d integers on the points' device" % n)
    return coded, U, n, lengths


class _SirenCodeFunction(torch.autograd.Function):
    """_SirenFunction with one latent code per cloud: the evaluation is iso_siren_sdf_grad_coded on `table` (U, H), the
    layer-0 biases of the codes as the no-grad route folds them (PackedSiren.fold); the backward is iso_sirencode_backward
    with `tail` (U, H), what that table lost against the float64 fold.  The gradient of the table, dt (U, model width), is
    handed to `t`, the caller's differentiable fold, whose values are not read: torch's chain over it delivers d codes, the
    code columns of d W_0 and d b_0.  The points are in packed order (code_of sorted, code_first the row starts); wb is
    W0x, W_1, b_1, .., W_L, b_L."""

    @staticmethod
    def forward(ctx, shape, need_grad, table, tail, code_of, code_first, t, pts, *wb):
        H, L, w0, wh = shape
        dev, n = pts.device, pts.shape[0]
        lib = _lib.load()
        if not lib.iso_sirengrad_form(H, L):
            raise RuntimeError("iso_points_amd: no fused SIREN backward for hidden %d, %d hidden layers" % (H, L))
        full = (wb[0], wb[0].new_zeros((wb[0].shape[0],))) + tuple(wb[1:])        # b_0 is not read: the table holds it
        packed = _pack_raw(_padded_raw(full, H, dev), H, L)
        sdf = torch.empty((n,), dtype=torch.float32, device=dev)
        grad = torch.empty((n, 3) if need_grad else (0, 3), dtype=torch.float32, device=dev)
        ws = torch.empty((lib.iso_project_siren_workspace_bytes(n, H, L),), dtype=torch.uint8, device=dev)
        _lib.call("iso_siren_sdf_grad_coded", _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(grad) if need_grad else None, n,
                  _lib.ptr(packed), H, L, w0, wh, _lib.ptr(ws), ws.numel(), _lib.stream(), _lib.ptr(table), _lib.ptr(code_of),
                  table.shape[0])
        ctx.shape, ctx.need_grad = shape, need_grad
        ctx.save_for_backward(table, tail, code_of, code_first, pts, *wb)
        ctx.set_materialize_grads(False)
        if not need_grad:
            ctx.mark_non_differentiable(grad)
        return sdf, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sdf, g_grad):
        H, L, w0, wh = ctx.shape
        table, tail, code_of, code_first, pts = ctx.saved_tensors[:5]
        wb = ctx.saved_tensors[5:]
        dev, n, U = pts.device, pts.shape[0], table.shape[0]
        need = ctx.needs_input_grad                      # .. 6: t, 7: pts, 8: W0x, 9..: W_1, b_1, ..
        if g_sdf is None and (g_grad is None or not ctx.need_grad):
            return (None,) * len(need)
        lib = _lib.load()
        full = (wb[0], wb[0].new_zeros((wb[0].shape[0],))) + tuple(wb[1:])
        raw = _padded_raw(full, H, dev)
        packed = _pack_raw(raw, H, L)
        u = torch.zeros((n,), dtype=torch.float32, device=dev) if g_sdf is None else \
            g_sdf.reshape(n).to(torch.float32).contiguous()
        v = g_grad.reshape(n, 3).to(torch.float32).contiguous() if (ctx.need_grad and g_grad is not None) else None
        g_pts = torch.empty_like(pts) if need[7] else None
        g_raw = torch.empty_like(raw) if any(need[8:]) else None      # NULL: no dW / db work is done
        g_tab = torch.empty_like(table) if need[6] else None
        ws = torch.empty((lib.iso_sirencode_workspace_bytes(n, H, L, U),), dtype=torch.uint8, device=dev)
        _lib.call("iso_sirencode_backward", _lib.ptr(pts), _lib.ptr(u), _lib.ptr(v), n, _lib.ptr(packed), H, L, w0, wh,
                  _lib.ptr(table), _lib.ptr(tail), _lib.ptr(code_of), _lib.ptr(code_first), U, _lib.ptr(g_raw), _lib.ptr(g_tab),
                  _lib.ptr(g_pts), _lib.ptr(ws), ws.numel(), _lib.stream())
        Hm = wb[0].shape[0]
        grads, at, nl = [], 0, len(full) // 2
        for i in range(nl):
            w, b = full[2 * i], full[2 * i + 1]
            rows = H if i < nl - 1 else w.shape[0]
            cols = H if i > 0 else w.shape[1]
            k = 8 + 2 * i - (1 if i > 0 else 0)          # b_0 is no input
            grads.append(g_raw[at:at + rows * cols].reshape(rows, cols)[:w.shape[0], :w.shape[1]].to(w.dtype)
                         if need[k] else None)
            at += rows * cols
            if i > 0:
                grads.append(g_raw[at:at + rows][:b.shape[0]].to(b.dtype) if need[k + 1] else None)
            at += rows
        return (None,) * 6 + (g_tab[:, :Hm] if need[6] else None, g_pts) + tuple(grads)


def _siren_forward_per_cloud(model, points, c, need_grad, cloud_idx, lengths):
    coded, U, n, lengths = _per_cloud_arguments(model, points, c, cloud_idx, lengths)
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
    lins, w0, wh, C = coded
    dev, shp = points.device, points.shape
    train = torch.is_grad_enabled() and (any(p.requires_grad for p in model.parameters()) or points.requires_grad
                                         or c.requires_grad)
    codes = c.detach().to(device=dev, dtype=torch.float32).contiguous()
    if not train:
        code_of = rows_of(lengths, dev) if lengths is not None else \
            cloud_idx.reshape(-1).to(torch.int64).clamp(0, U - 1).to(torch.int32)
        return siren_sdf_and_grad(model, points, need_grad=need_grad, code=CodeRows(codes, code_of))
    pts = points.reshape(-1, 3).to(torch.float32)
    if lengths is not None:
        inverse, code_of = None, rows_of(lengths, dev)
        starts = [0]
        for x in lengths:
            starts.append(starts[-1] + x)
        code_first = torch.tensor(starts, dtype=torch.int64).to(dev)
    else:
        order, inverse, code_of, code_first = cloud_order(cloud_idx, U)
        pts = pts[order]
    Hm = lins[0].out_features
    H = next(h for h in (64, 128, 256) if h >= Hm)
    W0 = lins[0].weight
    # the fold in float64 under grad; the kernels evaluate the table of the no-grad route (iso_siren_fold_codes), so that
    # the values are its bits, and the backward gets what THAT table lost against float64, per row (b0_tail's role)
    t64 = lins[0].bias.double() + c.to(dev).double() @ W0[:, :C].double().t()
    with torch.no_grad():
        table = torch.empty((U, H), dtype=torch.float32, device=dev)
        _lib.call("iso_siren_fold_codes", _lib.ptr(W0[:, :C].detach().float().contiguous()),
                  _lib.ptr(lins[0].bias.detach().float().contiguous()), _lib.ptr(codes), _lib.ptr(table), Hm, H, C, U,
                  _lib.stream())
        tail = torch.zeros((U, H), dtype=torch.float32, device=dev)
        tail[:, :Hm] = (t64.detach() - table[:, :Hm].double()).to(torch.float32)
    wb = [W0[:, C:]] + [t for lin in lins[1:] for t in (lin.weight, lin.bias)]
    sdf, grad = _SirenCodeFunction.apply((H, len(lins) - 2, float(w0), float(wh)), bool(need_grad), table, tail, code_of,
                                         code_first, t64.to(torch.float32), pts.contiguous(), *wb)
    if inverse is not None:
        sdf, grad = sdf[inverse], (grad[inverse] if need_grad else grad)
    return sdf.view(shp[:-1]), (grad.view(shp) if need_grad else None)


_TORCH_WARNED = set()


def _warn_torch_route(model, why):
    key = (type(model).__name__, why)
    if key in _TORCH_WARNED:
        return
    _TORCH_WARNED.add(key)
    warnings.warn("iso_points_amd: no fused SIREN backward for %s (%s) -- siren_forward runs model.forward and torch autograd"
                  % (type(model).__name__, why), RuntimeWarning, stacklevel=3)


def _torch_forward(model, points, c, need_grad, train):
    """model.forward (+ autograd.grad for the gradient) on the GPU: the route of whatever the fused kernels do not run.
    A code of fewer dimensions than the points is repeated over the points of its row."""
    shp = points.shape
    if c is not None and c.numel() > 0 and c.ndim != points.ndim:
        c = c.reshape((c.shape[0],) + (1,) * (points.ndim - 2) + (c.shape[-1],)) if c.ndim > 1 else \
            c.reshape((1,) * (points.ndim - 1) + (-1,))
    if c is not None and c.numel() > 0:
        c = c.expand(shp[:-1] + (c.shape[-1],))
    kw = {"c": c} if (c is not None and c.numel() > 0) else {}
    with torch.enable_grad() if (train or need_grad) else torch.no_grad():
        p = points if points.requires_grad else points.detach().requires_grad_(need_grad)
        sdf = model.forward(p, **kw).sdf
        grad = None
        if need_grad:
            grad = torch.autograd.grad(sdf, p, torch.ones_like(sdf), create_graph=train, retain_graph=train)[0]
    sdf = sdf.reshape(shp[:-1])
    if not train:
        sdf, grad = sdf.detach(), (grad.detach() if grad is not None else None)
    return sdf, grad


def siren_forward(model, points, c=None, need_grad=True, *, cloud_idx=None, lengths=None):
    """sdf (...) and grad (..., 3) of `model` at points (..., 3) (grad None when need_grad is False), to TRAIN with.

    Under grad mode, when a parameter of the model, the points or the code require grad, the results carry a grad_fn: the
    fused evaluation with the fused backward (_SirenFunction) into every weight and bias, the points and -- for a
    latent-conditioned SIREN with ONE code for all points, c (C,) / (1, C) -- the code, whose fold into layer 0's bias is
    made in torch.  The outputs are those of the GEMM mode the library is in; the backward differentiates the f32-MFMA
    evaluation of the same network.  Otherwise this is siren_sdf_and_grad, bit for bit.  One code per batch row under
    grad, and any model siren_spec / coded_siren_spec refuse, take model.forward and torch autograd (one warning per model
    class).

    One code per cloud on the fused kernels, under grad too (the auto-decoder step; implicit_modeling.py:211-218 with
    `c, cloud_idx=pointclouds.packed_to_cloud_idx()` in place of the gathered codes): c (U, C) and EITHER lengths, a host
    sequence of U counts summing to the n points, the clouds in packed order (no sort, no host read), OR cloud_idx, an
    (n,) integer device tensor in any order (clamped into [0, U), ordered by a stable device argsort, run sorted, handed
    back in the caller's order).  Both is a ValueError, as a shape that does not fit, before any launch.  The gradients
    go into every parameter, the points and every code (iso_sirencode_backward: the table of folded biases is a leaf of
    the kernels, torch's chain over the fold does the rest); sdf and grad are bit-identical to the no-grad call.
    The call WITHOUT these keywords keeps its route on purpose: padded points (N, P, 3) with c (N, C) under grad still go
    to model.forward with the warning above; padded callers who want the fused route pass lengths=[P] * N."""
    if cloud_idx is not None or lengths is not None:
        return _siren_forward_per_cloud(model, points, c, need_grad, cloud_idx, lengths)
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
    has_c = c is not None and torch.is_tensor(c) and c.numel() > 0
    spec = siren_spec(model)
    coded = coded_siren_spec(model) if spec is None else None
    train = torch.is_grad_enabled() and (any(p.requires_grad for p in model.parameters()) or points.requires_grad
                                         or (has_c and c.requires_grad))
    if spec is not None and has_c:
        raise ValueError("a latent-conditioned SIREN needs its code, an unconditioned one takes none")
    if coded is not None and not has_c:
        raise ValueError("iso_points_amd: this SIREN is conditioned on a latent code (c_dim = %d): pass c" % coded[3])
    if spec is None and coded is None:
        _warn_torch_route(model, "not a SIREN the fused kernels run")
        return _torch_forward(model, points, c, need_grad, train)
    if not train:
        if spec is not None:
            return siren_sdf_and_grad(model, points, need_grad=need_grad)
        rows = points.shape[0] if points.ndim > 1 else 1
        code = code_rows(c, coded[3], [points.numel() // 3 // max(rows, 1)] * rows)
        if code is None:
            _warn_torch_route(model, "code shape outside the kernels'")
            return _torch_forward(model, points, c, need_grad, train)
        return siren_sdf_and_grad(model, points, need_grad=need_grad, code=code)
    b0_tail = None
    if spec is not None:
        lins, w0, wh = spec
        wb = [t for lin in lins for t in (lin.weight, lin.bias)]
    else:
        lins, w0, wh, C = coded
        if not (c.shape[-1] == C and c.numel() == C):
            _warn_torch_route(model, "one code per batch row")
            return _torch_forward(model, points, c, need_grad, train)
        # the fold in float64, rounded to f32 once (iso_siren_fold_codes' rule); what the rounding drops is the same for
        # every point and would not average out of the sums over the points: the backward gets it as b0_tail
        W0 = lins[0].weight
        b64 = lins[0].bias.double() + W0[:, :C].double() @ c.reshape(C).double()
        b0 = b64.to(torch.float32)
        b0_tail = (b64.detach() - b0.detach().double()).to(torch.float32)
        wb = [W0[:, C:], b0] + [t for lin in lins[1:] for t in (lin.weight, lin.bias)]
    Hm = lins[0].out_features
    H = next(h for h in (64, 128, 256) if h >= Hm)
    shp = points.shape
    pts = points.reshape(-1, 3).to(torch.float32).contiguous()
    sdf, grad = _SirenFunction.apply((H, len(lins) - 2, float(w0), float(wh)), bool(need_grad), b0_tail, pts, *wb)
    return sdf.view(shp[:-1]), (grad.view(shp) if need_grad else None)


def get_normals_from_grad(decoder, p_world, c=None, requires_grad=False, return_sdf=False, cloud_idx=None, lengths=None,
                          **kwargs):
    """DSS/models/implicit_modeling.py:250-277 for a decoder handed in: the not normalised normals at p_world (N, *, 3), the
    gradient of the SDF w.r.t. the points; with return_sdf also the sdf (N, *, 1).  requires_grad=True: the normals (and
    the sdf) backpropagate into the decoder and the points, through sdf_forward's fused backward for a SIREN or an IDR network;
    requires_grad=False: detached normals.  cloud_idx / lengths: one code per cloud, c (U, C), as siren_forward takes them
    (the reference's call at :211-218 on packed points).  Further forward kwargs take model.forward."""
    if kwargs:
        _warn_torch_route(decoder, "forward kwargs")
        with torch.enable_grad():
            p = p_world if p_world.requires_grad else p_world.detach().requires_grad_(True)
            sdf = decoder.forward(p, c=c, **kwargs).sdf
            normals = torch.autograd.grad(sdf, p, torch.ones_like(sdf), create_graph=requires_grad,
                                          retain_graph=requires_grad or return_sdf)[0]
        sdf = sdf.reshape(p_world.shape[:-1])
    else:
        # as the reference, the sdf handed back keeps its graph whether or not the normals do
        with torch.enable_grad() if (requires_grad or return_sdf) else torch.no_grad():
            sdf, normals = sdf_forward(decoder, p_world, c=c, need_grad=True, cloud_idx=cloud_idx, lengths=lengths)
    if not requires_grad:
        normals = normals.detach()
    if return_sdf:
        return normals, sdf.unsqueeze(-1)
    return normals


# ----------------------------------------------------------------------------- IDR-style SDF
def _effective_weight(lin):
    """Weight of a (possibly weight-normalised) nn.Linear: g * v / |v| (common.py:277-278)."""
    if hasattr(lin, "weight_g") and hasattr(lin, "weight_v"):
        v = lin.weight_v
        return v * (lin.weight_g / v.norm(dim=1, keepdim=True))
    par = getattr(lin, "parametrizations", None)
    if par is not None and hasattr(par, "weight"):
        return lin.weight                       # new-style parametrization recomputes on access
    return lin.weight


def idr_spec(model):
    """(weights, biases, hidden, n_layers, skip, n_freq) if `model` is an IDR-style SDF
    (DSS/models/common.py:220-310; also the oracle's IdrSDF) the fused kernel supports, else None."""
    try:
        if hasattr(model, "v") and hasattr(model, "g") and hasattr(model, "dims"):      # oracle IdrSDF
            n_lin = model.num_layers - 1
            Ws = [model.weight(l) for l in range(n_lin)]
            bs = [model.b[l] for l in range(n_lin)]
            F_ = model.F
            skip_in = tuple(model.skip_in)
        elif hasattr(model, "lin0") and hasattr(model, "skip_in") and hasattr(model, "num_layers"):
            n_lin = model.num_layers - 1
            lins = [getattr(model, "lin%d" % l) for l in range(n_lin)]
            Ws = [_effective_weight(l) for l in lins]
            bs = [l.bias for l in lins]
            d0 = Ws[0].shape[1]
            if model.embed_fn is None or (d0 - 3) % 6 != 0:
                return None
            F_ = (d0 - 3) // 6
            skip_in = tuple(model.skip_in)
            sp = getattr(model, "softplus", None)
            if sp is None or abs(float(sp.beta) - 100.0) > 0 or float(getattr(sp, "threshold", 20)) != 20:
                return None
        else:
            return None
        n_layers = n_lin - 1
        H = Ws[-1].shape[1]
        if len(skip_in) > 1 or H not in (128, 256, 512) or not (2 <= n_layers <= 12) or F_ > 10:
            return None
        skip = skip_in[0] if len(skip_in) == 1 else -1
        d0 = 3 + 6 * F_
        if Ws[0].shape[1] != d0 or Ws[-1].shape[0] != 1:
            return None
        for l in range(n_layers):
            want = H - d0 if (skip >= 1 and l == skip - 1) else H
            if Ws[l].shape[0] != want or (l > 0 and Ws[l].shape[1] != H):
                return None
        if skip == 0 or skip >= n_layers:
            return None
        return Ws, bs, H, n_layers, skip, F_
    except Exception:
        return None


class PackedIdr(object):
    """Device-side MFMA weight image of an IDR-style SDF (iso_idr_pack_weights)."""

    def __init__(self, model, device):
        spec = idr_spec(model)
        if spec is None:
            raise ValueError("model is not an IDR-style SDF the fused kernel supports")
        Ws, bs, self.hidden, self.n_layers, self.skip, self.n_freq = spec
        parts = []
        for W, b in zip(Ws, bs):
            parts += [W.detach().reshape(-1), b.detach().reshape(-1)]
        raw = torch.cat(parts).to(device=device, dtype=torch.float32).contiguous()
        lib = _lib.load()
        assert raw.numel() == lib.iso_idr_raw_floats(self.hidden, self.n_layers, self.skip, self.n_freq)
        self.packed = torch.empty((lib.iso_idr_packed_floats(self.hidden, self.n_layers),), dtype=torch.float32,
                                  device=device)
        _lib.call("iso_idr_pack_weights", _lib.ptr(raw), _lib.ptr(self.packed), self.hidden, self.n_layers,
                  self.skip, self.n_freq, _lib.stream())
        self._ws = None

    def workspace(self, n):
        need = _lib.load().iso_project_idr_workspace_bytes(int(n), self.hidden, self.n_layers)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=self.packed.device)
        return self._ws


def idr_sdf_and_grad(model, points, need_grad=True, packed=None):
    shp = points.shape
    pts = points.detach().reshape(-1, 3).float().contiguous()
    pk = packed if packed is not None else PackedIdr(model, pts.device)
    n = pts.shape[0]
    sdf = torch.empty((n,), dtype=torch.float32, device=pts.device)
    grad = torch.empty((n, 3), dtype=torch.float32, device=pts.device) if need_grad else None
    ws = pk.workspace(n)
    _lib.call("iso_idr_sdf_grad", _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(grad), n, _lib.ptr(pk.packed), pk.hidden,
              pk.n_layers, pk.skip, pk.n_freq, 100.0, _lib.ptr(ws), ws.numel(), _lib.stream())
    return sdf.view(shp[:-1]), (grad.view(shp) if need_grad else None)


# ----------------------------------------------------------------------------- training an IDR network on the fused kernels
def _idr_raw(wb, device):
    """The effective W_0, b_0, .., W_n, b_n as the kernels' raw vector (iso_idr_raw_floats: true shapes, no padding)"""
    return torch.cat([t.detach().to(device=device, dtype=torch.float32).reshape(-1) for t in wb]).contiguous()


def _idr_pack_raw(raw, H, nl, skip, F_):
    lib = _lib.load()
    assert raw.numel() == lib.iso_idr_raw_floats(H, nl, skip, F_)
    packed = torch.empty((lib.iso_idr_packed_floats(H, nl),), dtype=torch.float32, device=raw.device)
    _lib.call("iso_idr_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, nl, skip, F_, _lib.stream())
    return packed


class _IdrFunction(torch.autograd.Function):
    """sdf (n,) and grad (n, 3) of the fused evaluation (iso_idr_sdf_grad, in whichever GEMM mode the library is in), with the
    fused backward (csrc/idrgrad.hip, iso_idrgrad_backward: the f32-MFMA evaluation of the same network, differentiated) into
    the points and the EFFECTIVE weights and biases W_0, b_0, .., W_n, b_n: those are made under grad by the caller
    (_effective_weight, the oracle's model.weight(l)), so weight norm's g and v get their gradients from torch's own chain.
    Only the inputs are kept; the backward packs the weight image again.  need_grad False: value only, the second output is
    an empty, non-differentiable tensor."""

    @staticmethod
    def forward(ctx, shape, need_grad, pts, *wb):
        H, nl, skip, F_ = shape
        dev, n = pts.device, pts.shape[0]
        lib = _lib.load()
        if not lib.iso_idrgrad_form(H, nl, skip, F_):
            raise RuntimeError("iso_points_amd: no fused IDR backward for hidden %d, %d layers, skip %d, %d frequencies"
                               % (H, nl, skip, F_))
        packed = _idr_pack_raw(_idr_raw(wb, dev), H, nl, skip, F_)
        sdf = torch.empty((n,), dtype=torch.float32, device=dev)
        grad = torch.empty((n, 3) if need_grad else (0, 3), dtype=torch.float32, device=dev)
        ws = torch.empty((lib.iso_project_idr_workspace_bytes(n, H, nl),), dtype=torch.uint8, device=dev)
        _lib.call("iso_idr_sdf_grad", _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(grad) if need_grad else None, n, _lib.ptr(packed),
                  H, nl, skip, F_, 100.0, _lib.ptr(ws), ws.numel(), _lib.stream())
        ctx.shape, ctx.need_grad = shape, need_grad
        ctx.save_for_backward(pts, *wb)
        ctx.set_materialize_grads(False)
        if not need_grad:
            ctx.mark_non_differentiable(grad)
        return sdf, grad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sdf, g_grad):
        H, nl, skip, F_ = ctx.shape
        pts, wb = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dev, n = pts.device, pts.shape[0]
        need = ctx.needs_input_grad
        if g_sdf is None and (g_grad is None or not ctx.need_grad):
            return (None,) * len(need)
        lib = _lib.load()
        raw = _idr_raw(wb, dev)
        packed = _idr_pack_raw(raw, H, nl, skip, F_)
        u = torch.zeros((n,), dtype=torch.float32, device=dev) if g_sdf is None else \
            g_sdf.reshape(n).to(torch.float32).contiguous()
        v = g_grad.reshape(n, 3).to(torch.float32).contiguous() if (ctx.need_grad and g_grad is not None) else None
        g_pts = torch.empty_like(pts) if need[2] else None
        g_raw = torch.empty_like(raw) if any(need[3:]) else None      # NULL: no dW / db work is done
        ws = torch.empty((lib.iso_idrgrad_workspace_bytes(n, H, nl, skip, F_),), dtype=torch.uint8, device=dev)
        _lib.call("iso_idrgrad_backward", _lib.ptr(pts), _lib.ptr(u), _lib.ptr(v), n, _lib.ptr(raw), _lib.ptr(packed), H, nl,
                  skip, F_, 100.0, _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(ws), ws.numel(), _lib.stream())
        grads, at = [], 0
        for i, t in enumerate(wb):
            grads.append(g_raw[at:at + t.numel()].reshape(t.shape).to(t.dtype) if need[3 + i] else None)
            at += t.numel()
        return (None, None, g_pts) + tuple(grads)


def idr_forward(model, points, need_grad=True):
    """sdf (...) and grad (..., 3) of an IDR-style SDF (idr_spec) at points (..., 3) (grad None when need_grad is False), to
    TRAIN with.  Under grad mode, when a parameter of the model or the points require grad, the results carry a grad_fn: the
    fused evaluation with the fused backward (_IdrFunction) into every effective weight and bias -- and through torch's chain
    into weight norm's g and v -- and into the points.  The outputs are those of the GEMM mode the library is in; the backward
    differentiates the f32-MFMA evaluation of the same network.  Otherwise this is idr_sdf_and_grad, bit for bit."""
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
    train = torch.is_grad_enabled() and (any(p.requires_grad for p in model.parameters()) or points.requires_grad)
    if not train:
        return idr_sdf_and_grad(model, points, need_grad=need_grad)
    spec = idr_spec(model)                       # the effective weights, made under grad
    if spec is None:
        raise ValueError("model is not an IDR-style SDF the fused kernel supports")
    Ws, bs, H, nl, skip, F_ = spec
    wb = [t for W, b in zip(Ws, bs) for t in (W, b)]
    shp = points.shape
    pts = points.reshape(-1, 3).to(torch.float32).contiguous()
    sdf, grad = _IdrFunction.apply((H, nl, skip, F_), bool(need_grad), pts, *wb)
    return sdf.view(shp[:-1]), (grad.view(shp) if need_grad else None)


def sdf_forward(model, points, c=None, need_grad=True, cloud_idx=None, lengths=None):
    """siren_forward for a SIREN or a latent-conditioned SIREN, idr_forward for an IDR-style SDF (which takes no code), and
    siren_forward's torch route with its one warning for anything else: sdf (...) and grad (..., 3) to train with.
    cloud_idx / lengths go to siren_forward (one code per cloud)."""
    if siren_spec(model) is None and coded_siren_spec(model) is None:
        with torch.no_grad():
            is_idr = idr_spec(model) is not None
        if is_idr:
            if c is not None and torch.is_tensor(c) and c.numel() > 0:
                raise ValueError("iso_points_amd: an IDR-style SDF takes no latent code")
            return idr_forward(model, points, need_grad=need_grad)
    return siren_forward(model, points, c=c, need_grad=need_grad, cloud_idx=cloud_idx, lengths=lengths)


class FusedSdf(object):
    """`sdf(points) -> values` for the callers that only need the value: the `sdf` callable of
    RayTracing (levelset_sampling.py:831-1167), the proposal / secant evaluations of
    find_zero_crossing_between_point_pairs (:1262-1267, :1350-1353) and the ray candidates of
    combined_modeling.py:376-380.  The weight image is packed once per instance (build one per
    optimiser step); SIREN and IDR-style networks run forward-only fused kernels, an analytic
    sphere or any other nn.Module is evaluated with model.forward on the GPU."""

    def __init__(self, model, device):
        self.model = model
        self.kind, self.packed = "generic", None
        if siren_spec(model) is not None:
            self.kind, self.packed = "siren", PackedSiren(model, device)
        elif idr_spec(model) is not None:
            self.kind, self.packed = "idr", PackedIdr(model, device)
        elif coded_siren_spec(model) is not None:
            self.kind, self.packed = "coded_siren", PackedSiren(model, device)

    def __call__(self, points, **forward_kwargs):
        """points (...,3) -> sdf (...).  A latent-conditioned SIREN takes its code as c=: one for all points ((C,) /
        (1, C)), one per leading row of `points` ((N, C) / (N, 1, C)), or CodeRows; other shapes, and any other
        forward kwarg, go to model.forward."""
        if not points.is_cuda:
            raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
        if self.kind == "coded_siren" and set(forward_kwargs) <= {"c"}:
            c = forward_kwargs.get("c")
            if c is None or (torch.is_tensor(c) and c.numel() == 0):
                raise ValueError("iso_points_amd: this SIREN is conditioned on a latent code (c_dim = %d): pass c"
                                 % self.packed.c_dim)
            rows = points.shape[0] if points.ndim > 1 else 1
            code = c if isinstance(c, CodeRows) else \
                code_rows(c, self.packed.c_dim, [points.numel() // 3 // max(rows, 1)] * rows)
            if code is not None:
                return siren_sdf_and_grad(self.model, points, need_grad=False, packed=self.packed, code=code)[0]
        if forward_kwargs or self.kind in ("generic", "coded_siren"):
            with torch.no_grad():
                return self.model.forward(points.reshape(-1, 3), **forward_kwargs).sdf.reshape(points.shape[:-1])
        if self.kind == "siren":
            return siren_sdf_and_grad(self.model, points, need_grad=False, packed=self.packed)[0]
        return idr_sdf_and_grad(self.model, points, need_grad=False, packed=self.packed)[0]
