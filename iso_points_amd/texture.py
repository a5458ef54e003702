"""The texture network: colours for iso-points, ray hits and mesh vertices.

`RenderingNetwork` mirrors the forward definition of the reference's class (DSS/models/common.py:313-366: same
constructor arguments, attribute names `lin0..`, `embed_fn`, `c_dim`, `dim`, `num_layers`, same state-dict keys), and
`NeuralTexture` the row assembly of DSS/core/texture.py:130-162 on plain tensors.  `texture_rgb` runs both in ONE fused
forward kernel (csrc/texture.hip, iso_texture_rgb): the row [c | normal, point | e(view direction)] is assembled per tile
inside the kernel and the activations never leave the chip.  What the kernel does not cover (texture_spec is None:
other widths, other outputs, wider codes) and any forward kwarg it does not know take decoder.forward on the GPU, with one
warning per decoder class.  There is no CPU path.  Under grad mode the rows train: `_TextureFunction` pairs the forward kernel
with the backward of csrc/texgrad.hip (iso_texgrad_backward) into the weights, biases, codes, normals and points.

`vertex_colors` is Generator.estimate_colors (implicit_modeling.py:790-820) and `raytrace_image` the body of
Generator.raytrace_images (:951-1001) for one view, both on the package's own SDF, tracing and texture kernels.
"""
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from .sdf_models import NetOutput, _effective_weight

_MAX_C, _MAX_F, _MAX_LAYERS = 256, 6, 8


class _Embedder(object):
    """get_embedder(F) (common.py:168-217): [v, sin(v 2^0), cos(v 2^0), sin(v 2^1), ...], 3 + 6 F wide."""

    def __init__(self, num_frequencies):
        self.num_frequencies = int(num_frequencies)
        self.out_dim = 3 + 6 * self.num_frequencies
        self.freqs = [2.0 ** k for k in range(self.num_frequencies)]

    def __call__(self, x):
        parts = [x]
        for f in self.freqs:
            parts += [torch.sin(x * f), torch.cos(x * f)]
        return torch.cat(parts, -1)


class RenderingNetwork(nn.Module):
    """common.py:313-366.  `dim` is the width of the raw geometry part (9 = normal, point, view direction); the encoding
    of the view direction widens the input by 6 * num_frequencies, the code by c_dim."""

    def __init__(self, dim=9, out_dims=None, c_dim=256, hidden_size=512, n_layers=4, weight_norm=True,
                 num_frequencies=4, **kwargs):
        super().__init__()
        out_dims = OrderedDict(rgb=3) if out_dims is None else out_dims
        self.out_dim = sum(out_dims.values())
        self._out_dims = tuple(out_dims.values())
        self._out_fields = tuple(out_dims.keys())
        self.c_dim = c_dim
        dims = [dim + c_dim] + [hidden_size] * n_layers + [self.out_dim]
        self.embed_fn = None
        if num_frequencies > 0:
            self.embed_fn = _Embedder(num_frequencies)
            dims[0] += self.embed_fn.out_dim - 3
        self.dim = dims[0]
        self.num_layers = len(dims)
        for l in range(self.num_layers - 1):
            lin = nn.Linear(dims[l], dims[l + 1])
            if weight_norm:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    lin = nn.utils.weight_norm(lin)          # the reference's (old-style) keys: weight_g, weight_v
            setattr(self, "lin" + str(l), lin)
        self.relu = nn.ReLU()
        self.tanh = nn.Tanh()

    def forward(self, x, c=None, **kwargs):
        if c is not None and c.numel() > 0:
            assert x.ndim == c.ndim
            x = torch.cat([c, x], dim=-1)
        for l in range(self.num_layers - 1):
            x = getattr(self, "lin" + str(l))(x)
            if l < self.num_layers - 2:
                x = self.relu(x)
        x = self.tanh(x)
        out = dict(zip(self._out_fields, torch.split(x, self._out_dims, dim=-1)))
        if "rgb" in out:
            out["rgb"] = (out["rgb"] + 1) / 2.0
        return NetOutput(**out)


def _view_width(decoder):
    """Slots the decoder's embed_fn makes of a direction (0: it has none)."""
    fn = getattr(decoder, "embed_fn", None)
    if fn is None:
        return 0
    return int(fn(torch.zeros((1, 3))).shape[-1])


def texture_spec(decoder):
    """(weights, biases, hidden, n_layers, c_dim, geom, n_freq) if `decoder` is a RenderingNetwork (the reference's or
    ours, weight-normed in either style or plain) the fused kernel covers, else None.  geom = 6 ([normal, point]) or 3
    (point); n_freq = -1: the rows hold no view direction, 0: the raw direction, F: get_embedder(F) of it.  Read off
    decoder.dim = c_dim + geom + view slots; a plain 6-wide geometry part is [normal, point] without a view."""
    try:
        if not (hasattr(decoder, "lin0") and hasattr(decoder, "num_layers") and hasattr(decoder, "c_dim")) \
                or hasattr(decoder, "skip_in") or not isinstance(getattr(decoder, "relu", None), nn.ReLU):
            return None
        if tuple(decoder._out_fields) != ("rgb",) or tuple(decoder._out_dims) != (3,):
            return None
        n_lin = decoder.num_layers - 1
        lins = [getattr(decoder, "lin%d" % l) for l in range(n_lin)]
        Ws = [_effective_weight(l) for l in lins]
        bs = [l.bias for l in lins]
        n_layers, H, C, D0 = n_lin - 1, Ws[-1].shape[1], int(decoder.c_dim), int(decoder.dim)
        if H not in (256, 512) or not (1 <= n_layers <= _MAX_LAYERS) or not (0 <= C <= _MAX_C):
            return None
        if Ws[0].shape != (H, D0) or Ws[-1].shape[0] != 3 or any(W.shape != (H, H) for W in Ws[1:-1]):
            return None
        V = _view_width(decoder)
        if V:
            if (V - 3) % 6 or (V - 3) // 6 > _MAX_F:
                return None
            G, Fq = D0 - C - V, (V - 3) // 6
        elif D0 - C == 9:
            G, Fq = 6, 0
        else:
            G, Fq = D0 - C, -1
        if G not in (3, 6):
            return None
        return Ws, bs, H, n_layers, C, G, Fq
    except Exception:
        return None


class PackedTexture(object):
    """Device-side split-fp16 weight image of a RenderingNetwork (iso_texture_pack_weights) and the launch's workspace.
    The image is a snapshot: texture_rgb packs a fresh one on every call unless the caller hands one in."""

    def __init__(self, decoder, device):
        spec = texture_spec(decoder)
        if spec is None:
            raise ValueError("decoder is not a RenderingNetwork the fused texture kernel supports")
        Ws, bs, self.hidden, self.n_layers, self.c_dim, self.geom, self.n_freq = spec
        self.shape = (self.hidden, self.n_layers, self.c_dim, self.geom, self.n_freq)
        parts = []
        for W, b in zip(Ws, bs):
            parts += [W.detach().reshape(-1), b.detach().reshape(-1)]
        raw = torch.cat(parts).to(device=device, dtype=torch.float32).contiguous()
        lib = _lib.load()
        assert lib.iso_texture_form(*self.shape) > 0
        assert raw.numel() == lib.iso_texture_raw_floats(*self.shape)
        self.packed = torch.empty((lib.iso_texture_packed_floats(*self.shape),), dtype=torch.float32, device=device)
        _lib.call("iso_texture_pack_weights", _lib.ptr(raw), _lib.ptr(self.packed), *self.shape, _lib.stream())
        self._ws = None

    def workspace(self, n):
        need = _lib.load().iso_texture_workspace_bytes(int(n), *self.shape)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((need,), dtype=torch.uint8, device=self.packed.device)
        return self._ws


def texture_rows(decoder, points, normals=None, camera_centers=None, cloud_idx=None):
    """The decoder's input without the code, as NeuralTexture.forward builds it (texture.py:137-156): [normals, points]
    (points alone when normals is None), and with camera_centers the direction normalize(points - centre of the point's
    cloud), through decoder.embed_fn where it has one.  Plain torch, in the dtype of `points`."""
    p = points.reshape(-1, 3)
    x = p if normals is None else torch.cat([normals.reshape(-1, 3).to(p.dtype), p], dim=-1)
    if camera_centers is not None:
        cam = camera_centers.reshape(-1, 3).to(p.dtype)
        cam = cam[cloud_idx.reshape(-1).long()] if cloud_idx is not None else cam[:1]
        view = F.normalize(p.detach() - cam, dim=-1)
        if getattr(decoder, "embed_fn", None) is not None:
            view = decoder.embed_fn(view)
        x = torch.cat([x, view], dim=-1)
    return x


_TORCH_WARNED = set()


def _warn_torch_route(decoder, why):
    key = (type(decoder).__name__, why)
    if key in _TORCH_WARNED:
        return
    _TORCH_WARNED.add(key)
    warnings.warn("iso_points_amd: no fused texture kernel for %s (%s) -- texture_rgb runs decoder.forward in torch"
                  % (type(decoder).__name__, why), RuntimeWarning, stacklevel=3)


def _launch_rgb(shape, packed, ws, pts, nrm, codes, cams, origin_of):
    n = pts.shape[0]
    rgb = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    _lib.call("iso_texture_rgb", _lib.ptr(pts), _lib.ptr(nrm), _lib.ptr(codes), _lib.ptr(cams), _lib.ptr(origin_of),
              0 if cams is None else cams.shape[0], _lib.ptr(rgb), n, _lib.ptr(packed), *shape, _lib.ptr(ws), ws.numel(),
              _lib.stream())
    return rgb


def _raw_of(wb, device):
    """The effective weights and biases W_0, b_0, ..., W_n, b_n as the kernels' raw vector."""
    return torch.cat([t.detach().reshape(-1) for t in wb]).to(device=device, dtype=torch.float32).contiguous()


class _TextureFunction(torch.autograd.Function):
    """rgb of the fused forward kernel, with the fused backward (csrc/texgrad.hip, iso_texgrad_backward) into the points,
    normals, codes and the EFFECTIVE weights and biases: those are made under grad by the caller, so weight_g / weight_v
    of either weight-norm style get their gradients from torch's own chain.  Only the inputs are kept for the backward,
    which recomputes the forward from them: the forward packs its split-fp16 image, the backward that image again and its own transposed
    one (iso_texgrad_pack_weights) from the same tensors, and neither image outlives its call."""

    @staticmethod
    def forward(ctx, shape, pts, nrm, codes, cams, origin_of, *wb):
        lib = _lib.load()
        dev = pts.device
        raw = _raw_of(wb, dev)
        packed = torch.empty((lib.iso_texture_packed_floats(*shape),), dtype=torch.float32, device=dev)
        _lib.call("iso_texture_pack_weights", _lib.ptr(raw), _lib.ptr(packed), *shape, _lib.stream())
        ws = torch.empty((lib.iso_texture_workspace_bytes(pts.shape[0], *shape),), dtype=torch.uint8, device=dev)
        ctx.shape = shape
        ctx.save_for_backward(pts, nrm, codes, cams, origin_of, *wb)
        return _launch_rgb(shape, packed, ws, pts, nrm, codes, cams, origin_of)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_rgb):
        lib = _lib.load()
        shape = ctx.shape
        pts, nrm, codes, cams, origin_of = ctx.saved_tensors[:5]
        wb = ctx.saved_tensors[5:]
        dev, n = pts.device, pts.shape[0]
        raw = _raw_of(wb, dev)
        packed_fw = torch.empty((lib.iso_texture_packed_floats(*shape),), dtype=torch.float32, device=dev)
        _lib.call("iso_texture_pack_weights", _lib.ptr(raw), _lib.ptr(packed_fw), *shape, _lib.stream())
        packed_bw = torch.empty((lib.iso_texgrad_packed_floats(*shape),), dtype=torch.float32, device=dev)
        _lib.call("iso_texgrad_pack_weights", _lib.ptr(raw), _lib.ptr(packed_bw), *shape, _lib.stream())
        need = ctx.needs_input_grad
        g_pts = torch.empty_like(pts) if need[1] else None
        g_nrm = torch.empty_like(nrm) if (need[2] and nrm is not None) else None
        g_codes = torch.empty_like(codes) if (need[3] and codes is not None) else None
        g_raw = torch.empty_like(raw) if any(need[6:]) else None      # NULL: no dW / db work is done
        ws = torch.empty((lib.iso_texgrad_workspace_bytes(n, *shape),), dtype=torch.uint8, device=dev)
        g = grad_rgb.reshape(n, 3).to(torch.float32).contiguous()
        _lib.call("iso_texgrad_backward", _lib.ptr(pts), _lib.ptr(nrm), _lib.ptr(codes), _lib.ptr(cams), _lib.ptr(origin_of),
                  0 if cams is None else cams.shape[0], _lib.ptr(g), n, _lib.ptr(packed_fw), _lib.ptr(packed_bw), *shape,
                  _lib.ptr(g_raw),
                  _lib.ptr(g_pts), _lib.ptr(g_nrm), _lib.ptr(g_codes), _lib.ptr(ws), ws.numel(), _lib.stream())
        grads, at = [], 0
        for k, t in enumerate(wb):
            grads.append(g_raw[at:at + t.numel()].reshape(t.shape).to(t.dtype) if need[6 + k] else None)
            at += t.numel()
        return (None, g_pts, g_nrm, g_codes, None, None) + tuple(grads)


def _wants_grad(decoder, *tensors):
    if not torch.is_grad_enabled():
        return False
    return any(p.requires_grad for p in decoder.parameters()) or any(t is not None and t.requires_grad for t in tensors)


def texture_rgb(decoder, points, normals=None, c=None, camera_centers=None, cloud_idx=None, packed=None, **forward_kwargs):
    """rgb (..., 3) in [0, 1] of decoder([c, normals, points, e(view direction)]) at points (..., 3).

    normals (..., 3) or None (rows of points alone); c (..., c_dim) or None; camera_centers (B, 3) / (3,) or None (no view
    direction); cloud_idx (...) integer, the row of camera_centers a point looks from (None: row 0).  What is passed must
    add up to decoder.dim.  packed: a PackedTexture of this decoder to re-use -- on the caller's word that the weights have
    not changed since; by default the image is packed from the live weights on every call.  A decoder texture_spec refuses,
    and any further forward kwarg, takes decoder.forward on the rows of texture_rows (one warning per decoder class).

    Under grad mode, with a parameter of the decoder or one of points / normals / c requiring grad and packed None, the
    result carries a grad_fn: the fused backward kernels give the gradients of every weight and bias (through the
    weight-norm parameters, where there are any), of the codes, the normals and the points; as in the reference the view
    direction is detached and camera_centers get none.  A caller's `packed` image is a snapshot of the weights and stays
    inference-only: the result then has no grad_fn.  The torch route keeps its graph when a gradient is wanted."""
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
    shp = points.shape
    n = points.numel() // 3
    has_c = c is not None and c.numel() > 0
    spec = texture_spec(decoder) if packed is None else True
    train = packed is None and _wants_grad(decoder, points, normals, c if has_c else None)
    if spec is None or forward_kwargs:
        _warn_torch_route(decoder, "forward kwargs" if spec is not None else "shape outside the kernel's")
        with torch.enable_grad() if train else torch.no_grad():
            x = texture_rows(decoder, points, normals, camera_centers, cloud_idx)
            cc = c.reshape(n, -1).to(x.dtype) if has_c else None
            return decoder.forward(x, c=cc, **forward_kwargs).rgb.reshape(shp[:-1] + (3,))
    if train:
        Ws, bs = spec[0], spec[1]
        pk = None
        pk_c, pk_g, pk_f = spec[4:7]
        kshape = tuple(spec[2:7])
    else:
        pk = packed if packed is not None else PackedTexture(decoder, points.device)
        pk_c, pk_g, pk_f = pk.c_dim, pk.geom, pk.n_freq
        kshape = pk.shape
    G = 3 if normals is None else 6
    Fq = -1 if camera_centers is None else max(pk_f, 0)
    C = c.shape[-1] if has_c else 0
    if (C, G, Fq) != (pk_c, pk_g, pk_f):
        raise ValueError("texture_rgb: the decoder takes rows of (c_dim, geometry, n_freq) = %s, the arguments make %s"
                         % ((pk_c, pk_g, pk_f), (C, G, Fq)))
    dev = points.device

    def dense(t, width):
        t = (t if train else t.detach()).reshape(-1, width).to(device=dev, dtype=torch.float32).contiguous()
        if t.shape[0] != n:
            raise ValueError("texture_rgb: %d rows for %d points" % (t.shape[0], n))
        return t
    pts = dense(points, 3)
    nrm = dense(normals, 3) if normals is not None else None
    codes = dense(c, C) if has_c else None
    cams = origin_of = None
    n_origins = 0
    if camera_centers is not None:
        cams = camera_centers.detach().reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
        n_origins = cams.shape[0]
        if cloud_idx is not None:
            origin_of = cloud_idx.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
            if origin_of.shape[0] != n:
                raise ValueError("texture_rgb: %d cloud indices for %d points" % (origin_of.shape[0], n))
    if train:
        wb = [t for pair in zip(Ws, bs) for t in pair]
        rgb = _TextureFunction.apply(kshape, pts, nrm, codes, cams, origin_of, *wb)
    else:
        rgb = _launch_rgb(kshape, pk.packed, pk.workspace(n), pts, nrm, codes, cams, origin_of)
    return rgb.reshape(shp[:-1] + (3,))


class NeuralTexture(nn.Module):
    """DSS/core/texture.py:130-162 on packed tensors: forward returns the rgb rows (the reference writes them into a clone
    of its point-cloud container)."""

    def __init__(self, decoder, view_dependent=True):
        super().__init__()
        self.view_dependent = view_dependent
        self.decoder = decoder

    def forward(self, points, normals=None, c=None, camera_centers=None, lengths=None, cloud_idx=None, packed=None,
                **kwargs):
        """points (n, 3) packed; normals (n, 3); c (n, c_dim); camera_centers (B, 3); the cloud of a point either as
        cloud_idx (n,) or as lengths (B,), the clouds' sizes in packed order (a device tensor of lengths is read back)."""
        if cloud_idx is None and lengths is not None:
            lens = torch.as_tensor(lengths).reshape(-1).to(points.device)
            cloud_idx = torch.repeat_interleave(torch.arange(lens.numel(), device=points.device), lens)
        if self.decoder.dim == 3 and not self.view_dependent:                     # :137-138
            return texture_rgb(self.decoder, points, None, c, None, None, packed, **kwargs)
        assert normals is not None                                                # :141
        cams = camera_centers if self.view_dependent else None                   # :145-156
        return texture_rgb(self.decoder, points, normals, c, cams, cloud_idx if cams is not None else None, packed, **kwargs)


def _sdf_gradient(sdf, pts):
    """SDF gradient (not normalised) at pts (n, 3): the fused gradient kernel where the model has one, autograd otherwise."""
    from .ops import _fused
    from .sdf_models import FusedSdf, idr_sdf_and_grad, siren_sdf_and_grad
    fused = _fused(sdf, pts.device)
    if fused is not None:
        grad_fn = siren_sdf_and_grad if fused.kind == "siren" else idr_sdf_and_grad
        return grad_fn(fused.model, pts, need_grad=True, packed=fused.packed)[1]
    fn = sdf.model if isinstance(sdf, FusedSdf) else sdf
    with torch.enable_grad():
        x = pts.detach().clone().requires_grad_(True)
        val = fn(x)
        return torch.autograd.grad(getattr(val, "sdf", val).sum(), x)[0]


def _packed_or_none(texture, device):
    return PackedTexture(texture.decoder, device) if texture_spec(texture.decoder) is not None else None


def vertex_colors(sdf, texture, verts, c=None, with_normals=True, camera_centers=None, points_batch_size=100000):
    """Generator.estimate_colors (implicit_modeling.py:790-820): the texture at mesh vertices verts (V, 3), in chunks of
    points_batch_size, clipped to [0, 1].  with_normals: the SDF gradient at the vertices (the fused gradient kernels for a
    SIREN / IDR model) as the normal part of the rows.  texture: a NeuralTexture; c (V, c_dim) or None.  The weights are
    packed once for all chunks."""
    if not verts.is_cuda:
        raise RuntimeError("iso_points_amd: verts must be on the GPU; there is no CPU path")
    verts = verts.detach().reshape(-1, 3).float()
    packed = _packed_or_none(texture, verts.device)
    out = []
    with torch.no_grad():
        for lo in range(0, verts.shape[0], int(points_batch_size)):
            part = verts[lo:lo + int(points_batch_size)].contiguous()
            normals = _sdf_gradient(sdf, part) if with_normals else None
            ci = c[lo:lo + int(points_batch_size)] if c is not None else None
            out.append(texture(part, normals, c=ci, camera_centers=camera_centers, packed=packed).clamp(0.0, 1.0))
    return torch.cat(out) if out else verts.new_zeros((0, 3))


def raytrace_image(sdf, texture, camera_center, ray_directions, object_mask, ray_tracer=None):
    """One view of Generator.raytrace_images (implicit_modeling.py:951-1001): RayTracing.forward finds the hits, the SDF
    gradient at the hits is their normal, NeuralTexture their colour.  camera_center (3,); ray_directions (R, 3) unit;
    object_mask (R,) bool.  Returns rgba (R, 4) float32: colour and 1 on the rays that hit, zeros elsewhere.
    ray_tracer: a RayTracing (default: RayTracing() in eval mode, as the reference's validation step runs it).
    One host read of this function's own: the hit list (torch.nonzero of the tracer's mask), so that gradient and texture
    run on the compacted hits only."""
    from .ray_tracing import RayTracing
    from .sdf_models import FusedSdf
    if not ray_directions.is_cuda:
        raise RuntimeError("iso_points_amd: rays must be on the GPU; there is no CPU path")
    dev = ray_directions.device
    dirs = ray_directions.reshape(1, -1, 3).float()
    cam = camera_center.reshape(1, 3).to(device=dev, dtype=torch.float32)
    tracer = ray_tracer if ray_tracer is not None else RayTracing().eval()
    value = sdf if isinstance(sdf, FusedSdf) else FusedSdf(sdf, dev)
    with torch.no_grad():
        pts, mask, _ = tracer(value, cam, object_mask.reshape(-1).to(dev), dirs)
        rgba = torch.zeros((dirs.shape[1], 4), dtype=torch.float32, device=dev)
        rows = torch.nonzero(mask.reshape(-1), as_tuple=False).flatten()         # the host read
        if rows.numel() > 0:
            hits = pts.reshape(-1, 3)[rows].contiguous()
            rgb = texture(hits, _sdf_gradient(value, hits), camera_centers=cam)
            rgba[rows, :3] = rgb
            rgba[rows, 3] = 1.0
    return rgba
