"""Chamfer distance between point clouds: pytorch3d.loss.chamfer_distance as the reference calls it
(evaluation.py:119-122 and :169-172 -- chamfer_p / chamfer_n; DSS/training/trainer.py:256 -- the validation
metric train_mvr.py:196 selects checkpoints by), and the distances between point clouds and mesh faces:
pytorch3d.loss.point_mesh_face_distance (evaluation.py:123-126, :173-176 -- pf_dist) and
pytorch3d.loss.point_mesh_distance.point_face_distance (DSS/training/losses.py:536-598, SignedDistanceLoss), and the sign
that loss gives the distance: point_mesh_sign / point_mesh_signed_distance / mesh_pseudonormals, an exact inside test by
angle-weighted pseudonormals in place of the reference's raster parity (include/isopoints.h section J).

The point-cloud regularisers of the splatting renderer, ProjectionLoss and RepulsionLoss (DSS/training/losses.py:149-515),
are surface_losses and the two modules on it: one search for the 32 nearest other points, two fused normal mollifications
and one fused sweep that returns both losses with their gradients (include/isopoints.h section K).  The third, NormalLoss
(:86-102), compares the points' normals with the PCA normals of math_helper and reaches the positions through the
local-frame kernel's backward (iso_pca_frames_backward).

The nearest-point search runs on the cell grid of iso_points_amd.frnn (exact, any distance), fused with the
normal term and the per-cloud sums; the backward pass is a gather over counting-sorted index lists.  Neither
uses float atomics: values and gradients are the same bits from run to run (include/isopoints.h section G).
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib
from . import frnn
from .levelset_sampling import convert_pointclouds_to_tensor, host_lengths, padded_to_packed, with_host_lengths

_INF = float("inf")


def _grid_of(points, lengths):
    """The grid knn_points builds for K = 1: infinite radius, 8 points per occupied cell."""
    r = torch.full((points.shape[0],), _INF, dtype=torch.float32, device=points.device)
    return frnn.build_grid(points, lengths, r, points_per_cell=8.0)


def _nearest(x, y, x_len, y_len, x_normals=None, y_normals=None, rows=True):
    """One direction.  x, y float32 contiguous on the GPU, lengths int64 on the GPU.  Returns d2 (N,P1), idx (N,P1) int32,
    normal term (N,P1) or None, sums (N,2) = per-cloud {sum d2, sum normal term}; rows=False leaves d2 and the normal
    term unwritten (None): the loss needs the indices and the sums only."""
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    dev = x.device
    grid = _grid_of(y, y_len)
    d2 = torch.empty((N, P1), dtype=torch.float32, device=dev) if rows else None
    idx = torch.empty((N, P1), dtype=torch.int32, device=dev)
    nterm = torch.empty((N, P1), dtype=torch.float32, device=dev) if rows and x_normals is not None else None
    sums = torch.empty((N, 2), dtype=torch.float32, device=dev)
    ws_bytes = _lib.load().iso_chamfer_nearest_workspace_bytes(N, P1, P2)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.call("iso_chamfer_nearest", p(x), p(x_len), p(grid.sorted_points), p(grid.sorted_idx), p(y_len), p(grid.off),
              p(grid.params), p(x_normals), p(y_normals), p(d2), p(idx), p(nterm), p(sums), N, P1, P2, grid.g_stride,
              p(ws), ws_bytes, _lib.stream())
    return d2, idx, nterm, sums


class _ChamferSums(torch.autograd.Function):
    """(x, y, normals) -> per-cloud sums of the squared nearest distances and of the normal terms, both directions."""

    @staticmethod
    def forward(ctx, x, y, x_normals, y_normals, x_len, y_len):
        _, idx_x, _, sums_x = _nearest(x, y, x_len, y_len, x_normals, y_normals, rows=False)
        _, idx_y, _, sums_y = _nearest(y, x, y_len, x_len, y_normals, x_normals, rows=False)
        ctx.save_for_backward(x, y, x_normals, y_normals, x_len, y_len, idx_x, idx_y)
        return sums_x[:, 0], sums_y[:, 0], sums_x[:, 1], sums_y[:, 1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dx, g_dy, g_nx, g_ny):
        x, y, x_normals, y_normals, x_len, y_len, idx_x, idx_y = ctx.saved_tensors
        need_x, need_y, need_xn, need_yn = ctx.needs_input_grad[:4]
        normals = x_normals is not None
        need_xn, need_yn = need_xn and normals, need_yn and normals
        # only what is asked for: the trainer's ground-truth cloud costs nothing; a normal gradient rides on its cloud's side
        grad_x = torch.empty_like(x) if (need_x or need_xn) else None
        grad_y = torch.empty_like(y) if (need_y or need_yn) else None
        grad_xn = torch.empty_like(x_normals) if need_xn else None
        grad_yn = torch.empty_like(y_normals) if need_yn else None
        if grad_x is None and grad_y is None:
            return None, None, None, None, None, None
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]

        def scale(g):
            return g.detach().float().contiguous()
        ws_bytes = _lib.load().iso_chamfer_backward_workspace_bytes(N, P1, P2)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
        p = _lib.ptr
        want_n = need_xn or need_yn
        _lib.call("iso_chamfer_backward", p(x), p(y), p(x_len), p(y_len), p(idx_x), p(idx_y), p(scale(g_dx)), p(scale(g_dy)),
                  p(x_normals), p(y_normals), p(scale(g_nx)) if want_n else None, p(scale(g_ny)) if want_n else None,
                  p(grad_x), p(grad_y), p(grad_xn), p(grad_yn), N, P1, P2, p(ws), ws_bytes, _lib.stream())
        return (grad_x if need_x else None), (grad_y if need_y else None), grad_xn, grad_yn, None, None


def _clouds(points, lengths, normals, what):
    """Validated (points (N,P,3), lengths (N,) int64, normals or None) of one cloud argument, still on their own device."""
    pts, conv_len = convert_pointclouds_to_tensor(points)
    if pts.dim() != 3 or pts.shape[-1] != 3:
        raise ValueError("chamfer_distance: %s must be (N, P, 3), got %s" % (what, tuple(pts.shape)))
    if lengths is None:
        lengths = conv_len
    lengths = torch.as_tensor(lengths)
    # the range check reads the lengths on the host: the host copy where the tensor carries one (full_lengths and every
    # lengths tensor this package returns), so that only lengths built by the caller on the GPU cost a device read.  Taken
    # before any reshape: the host copy rides on this very tensor
    host = host_lengths(lengths)
    if lengths.dim() != 1:
        lengths = lengths.reshape(-1)
    if lengths.shape[0] != pts.shape[0]:
        raise ValueError("chamfer_distance: %s_lengths must have one entry per cloud" % what)
    if any(l > pts.shape[1] or l < 0 for l in host):
        raise ValueError("chamfer_distance: %s_lengths must lie in [0, %d]" % (what, pts.shape[1]))
    lengths = lengths.to(torch.int64)
    if normals is not None and tuple(normals.shape) != tuple(pts.shape):
        raise ValueError("chamfer_distance: %s_normals must have the shape of %s" % (what, what))
    return pts, lengths, normals


def _on_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("iso_points_amd.loss: tensors must be on the GPU; there is no CPU path")


def nearest_points(x, y, x_lengths=None, y_lengths=None):
    """For every point of x the exact nearest point of y: (d2 (N,P1) f32, idx (N,P1) int64), d2 = (dx*dx + dy*dy) + dz*dz in
    f32, ties to the lower index; rows beyond x_lengths hold d2 = 0, idx = -1.  No gradient."""
    x, x_len, _ = _clouds(x, x_lengths, None, "x")
    y, y_len, _ = _clouds(y, y_lengths, None, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError("nearest_points: x and y must have the same batch size")
    _on_gpu(x, y)
    dev = x.device
    d2, idx, _, _ = _nearest(x.detach().float().contiguous(), y.detach().float().contiguous(),
                             x_len.to(dev).contiguous(), y_len.to(dev).contiguous())
    return d2, idx.long()


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction="mean", point_reduction="mean"):
    """pytorch3d.loss.chamfer_distance: (cham_dist, cham_normals); cham_normals is None without normals.

    Per cloud, cham_x = sum_i min_j |x_i - y_j|^2 (divided by x_lengths for point_reduction "mean"), cham_y likewise, each
    times weights[n]; then the batch is summed ("sum"), summed and divided by weights.sum() (N without weights; "mean") or
    kept as an (N,) vector (None).  The normal term is 1 - |cos| between a point's normal and its nearest point's.
    Differentiable w.r.t. x, y, x_normals, y_normals; nearest indices are constants.  All arithmetic is float32: other
    floating dtypes are cast on the way in, the results are float32 and the gradients arrive in the input's dtype with
    float32 precision.  Without `weights` and with lengths that carry a host copy (or none) the call reads nothing back
    from the device; `weights` cost one read each for pytorch3d's two checks (negative, all zero)."""
    if batch_reduction is not None and batch_reduction not in ("mean", "sum"):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if (x_normals is None) != (y_normals is None):
        raise ValueError("chamfer_distance: normals must be given for both clouds or for neither")
    x, x_len, x_normals = _clouds(x, x_lengths, x_normals, "x")
    y, y_len, y_normals = _clouds(y, y_lengths, y_normals, "y")
    N = x.shape[0]
    if y.shape[0] != N:
        raise ValueError("chamfer_distance: x and y must have the same batch size")
    if weights is not None:
        if weights.dim() != 1 or weights.shape[0] != N:
            raise ValueError("chamfer_distance: weights must be of shape (N,)")
        if not bool((weights >= 0).all()):
            raise ValueError("chamfer_distance: weights cannot be negative")
    _on_gpu(x, y, x_normals, y_normals, weights)
    dev = x.device
    normals = x_normals is not None

    def f32(t):
        return t.float().contiguous() if t is not None else None
    x_len, y_len = x_len.to(dev).contiguous(), y_len.to(dev).contiguous()
    cham_x, cham_y, norm_x, norm_y = _ChamferSums.apply(f32(x), f32(y), f32(x_normals), f32(y_normals), x_len, y_len)

    if weights is not None and not bool(weights.any()):
        # pytorch3d's early return: zeros that still reach the inputs, with a zero gradient
        def zero(a, b):
            z = (a + b) * weights.float() * 0.0
            return z if batch_reduction is None else z.sum()
        return zero(cham_x, cham_y), (zero(norm_x, norm_y) if normals else None)

    def reduce(sx, sy):
        if point_reduction == "mean":
            sx = sx / x_len.clamp(min=1).float()
            sy = sy / y_len.clamp(min=1).float()
        if weights is not None:
            sx, sy = sx * weights.float(), sy * weights.float()
        if batch_reduction is not None:
            sx, sy = sx.sum(), sy.sum()
            if batch_reduction == "mean":
                div = weights.float().sum() if weights is not None else float(N)
                sx, sy = sx / div, sy / div
        return sx + sy

    return reduce(cham_x, cham_y), (reduce(norm_x, norm_y) if normals else None)


# ------------------------------------------------------------------------------------------ point <-> mesh face distances
class _Segments(object):
    """The packed layout of a batch: per cloud and per mesh the first row and the row count, on the device (int64) and on
    the host; the strides are the longest cloud and the longest mesh (at least one row)."""

    def __init__(self, p_first, p_host, P, t_first, t_host, T, fn):
        if len(p_host) != len(t_host):
            raise ValueError("%s: points and tris must have the same batch size" % fn)
        self.N, self.P, self.T = len(p_host), P, T
        self.p_first, self.p_len, self.p_len_host = self._lengths(p_first, p_host, P, "points_first_idx", fn)
        self.t_first, self.t_len, self.t_len_host = self._lengths(t_first, t_host, T, "tris_first_idx", fn)
        self.p_stride = max(self.p_len_host + [1])
        self.t_stride = max(self.t_len_host + [1])

    @staticmethod
    def _lengths(first, host, total, what, fn):
        # a packed layout tiles its rows: the first cloud starts at row 0 and every cloud ends where the next one starts
        ends = host[1:] + [total]
        if host and (host[0] != 0 or any(e < f for f, e in zip(host, ends))):
            raise ValueError("%s: %s must start at 0, ascend and stay within the %d packed rows" % (fn, what, total))
        first = first.to(torch.int64)
        end = torch.full((1,), total, dtype=torch.int64, device=first.device)
        return first.contiguous(), (torch.cat([first[1:], end]) - first).contiguous(), [e - f for f, e in zip(host, ends)]

    def to(self, dev):
        for k in ("p_first", "p_len", "t_first", "t_len"):
            setattr(self, k, getattr(self, k).to(dev))
        return self


def _first_of(lengths, host):
    """first_idx of clouds of these lengths, with its host copy."""
    first, acc = [], 0
    for l in host:
        first.append(acc)
        acc += int(l)
    return with_host_lengths(torch.cumsum(lengths, 0) - lengths, first)


def _pf_search(direction, points, tris, seg, min_area):
    """One direction on validated float32 inputs: d2 (Q,) f32, idx (Q,) int32 packed, sums (N,) f32."""
    dev = points.device
    N, P, T = seg.N, seg.P, seg.T
    Q = P if direction == 0 else T
    cen = torch.empty((N, seg.t_stride, 3), dtype=torch.float32, device=dev)
    rad = torch.empty((max(T, 1),), dtype=torch.float32, device=dev)
    rmax = torch.empty((max(N, 1),), dtype=torch.float32, device=dev)
    pad = torch.empty((N, seg.p_stride, 3), dtype=torch.float32, device=dev) if direction == 1 else None
    d2 = torch.empty((Q,), dtype=torch.float32, device=dev)
    idx = torch.empty((Q,), dtype=torch.int32, device=dev)
    sums = torch.empty((N,), dtype=torch.float32, device=dev)
    if N == 0:
        return d2, idx, sums
    p = _lib.ptr
    _lib.call("iso_pfdist_prepare", p(points), p(seg.p_first), p(seg.p_len), p(tris), p(seg.t_first), p(seg.t_len), N, P, T,
              seg.p_stride, seg.t_stride, p(pad), p(cen), p(rad), p(rmax), _lib.stream())
    grid = _grid_of(cen, seg.t_len) if direction == 0 else _grid_of(pad, seg.p_len)
    strides = (seg.p_stride, seg.t_stride) if direction == 0 else (seg.t_stride, seg.p_stride)
    ws_bytes = _lib.load().iso_pfdist_forward_workspace_bytes(direction, N, *strides)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _lib.call("iso_pfdist_forward", direction, p(points), p(seg.p_first), p(seg.p_len), p(tris), p(seg.t_first),
              p(seg.t_len), p(grid.sorted_points), p(grid.sorted_idx), p(grid.off), p(grid.params), p(cen), p(rad), p(rmax),
              float(min_area), p(d2), p(idx), p(sums), N, P, T, seg.p_stride, seg.t_stride, grid.g_stride, p(ws), ws_bytes,
              _lib.stream())
    return d2, idx, sums


class _FaceDistance(torch.autograd.Function):
    """(points (P,3), tris (T,3,3)) -> the squared distance of every query of one direction to its nearest target, the
    per-cloud sums of them and the targets' packed indices (constants)."""

    @staticmethod
    def forward(ctx, points, tris, direction, min_area, seg):
        d2, idx, sums = _pf_search(direction, points, tris, seg, min_area)
        ctx.save_for_backward(points, tris, idx)
        ctx.direction, ctx.min_area, ctx.seg = direction, min_area, seg
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return d2, sums, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_d2, g_sums, _g_idx):
        points, tris, idx = ctx.saved_tensors
        need_p, need_t = ctx.needs_input_grad[:2]
        seg, direction = ctx.seg, ctx.direction
        Q = seg.P if direction == 0 else seg.T
        if not (need_p or need_t) or (g_d2 is None and g_sums is None) or Q == 0:
            return None, None, None, None, None
        # one weight per query: its own upstream gradient and its cloud's
        w = g_d2.detach().float() if g_d2 is not None else None
        if g_sums is not None:
            rows = seg.p_len if direction == 0 else seg.t_len
            per_cloud = torch.repeat_interleave(g_sums.detach().float(), rows, output_size=Q)
            w = per_cloud if w is None else w + per_cloud
        w = w.contiguous()
        # only what is asked for: a ground-truth mesh costs neither a buffer nor its lists
        grad_p = torch.empty_like(points) if need_p else None
        grad_t = torch.empty_like(tris) if need_t else None
        ws_bytes = _lib.load().iso_pfdist_backward_workspace_bytes(direction, seg.P, seg.T)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=points.device)
        p = _lib.ptr
        _lib.call("iso_pfdist_backward", direction, p(points), p(tris), p(idx), p(w), float(ctx.min_area), p(grad_p),
                  p(grad_t), seg.P, seg.T, p(ws), ws_bytes, _lib.stream())
        return grad_p, grad_t, None, None, None


def _pf_inputs(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area, fn):
    """Validated (points f32 (P,3), tris f32 (T,3,3), segments) of a packed call; ValueError before any GPU work."""
    for t, what in ((points, "points"), (tris, "tris"), (points_first_idx, "points_first_idx"),
                    (tris_first_idx, "tris_first_idx")):
        if not torch.is_tensor(t):
            raise ValueError("%s: %s must be a tensor" % (fn, what))
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("%s: points must be (P, 3), got %s" % (fn, tuple(points.shape)))
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
        raise ValueError("%s: tris must be (T, 3, 3), got %s" % (fn, tuple(tris.shape)))
    if points_first_idx.dim() != 1 or tris_first_idx.dim() != 1:
        raise ValueError("%s: points_first_idx and tris_first_idx must be of shape (N,)" % fn)
    if points_first_idx.is_floating_point() or tris_first_idx.is_floating_point():
        raise ValueError("%s: points_first_idx and tris_first_idx hold integer rows" % fn)
    if not float(min_triangle_area) >= 0.0:
        raise ValueError("%s: min_triangle_area must not be negative" % fn)
    seg = _Segments(points_first_idx, host_lengths(points_first_idx), points.shape[0], tris_first_idx,
                    host_lengths(tris_first_idx), tris.shape[0], fn)
    if max_points is not None and max(seg.p_len_host + [0]) > int(max_points):
        raise ValueError("%s: a cloud holds more than max_points = %d points" % (fn, int(max_points)))
    _on_gpu(points, tris)
    return points.float().contiguous(), tris.float().contiguous(), seg.to(points.device)


def point_face_distance(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area=0.0):
    """pytorch3d.loss.point_mesh_distance.point_face_distance: (P,) squared distances from every point of the packed
    clouds `points` (P,3) to the nearest face of its own mesh among the packed triangles `tris` (T,3,3);
    points_first_idx / tris_first_idx (N,) give each cloud's / mesh's first row.  A point whose mesh is empty gets 0.

    The distance to a face is |p - c|^2 at the closest point c of the closed triangle, in float32; a face whose area is
    <= min_triangle_area is measured by its three edges only (pytorch3d's current default is 5e-3, the version the
    reference pins has none: 0.0 here).  Differentiable w.r.t. points and tris with the nearest faces held constant;
    values and gradients are the same bits from run to run.  The search walks the cell grid of the faces' centroids and
    stops once the best distance is within the walked reach less the mesh's largest centroid-to-vertex distance: exact
    for any mesh, but one face far larger than the rest makes that radius large and drives every walk of its mesh toward
    a brute force."""
    pts, tr, seg = _pf_inputs(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area,
                              "point_face_distance")
    return _FaceDistance.apply(pts, tr, 0, float(min_triangle_area), seg)[0]


def face_point_distance(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area=0.0):
    """pytorch3d.loss.point_mesh_distance.face_point_distance: (T,) squared distances from every face to the nearest
    point of its own cloud; arguments, arithmetic and gradients as point_face_distance.  The search walks the cell grid
    of the points from the face's centroid and allows for the face's own radius."""
    pts, tr, seg = _pf_inputs(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area,
                              "face_point_distance")
    return _FaceDistance.apply(pts, tr, 1, float(min_triangle_area), seg)[0]


def nearest_faces(points, tris, points_first_idx=None, tris_first_idx=None, min_triangle_area=0.0):
    """For every point of `points` (P,3) the nearest face of `tris` (T,3,3): (d2 (P,) f32, idx (P,) int64 into tris), ties
    to the lower face index; without first_idx tensors one cloud against one mesh.  A point without faces gets d2 = 0,
    idx = -1.  No gradient."""
    if (points_first_idx is None) != (tris_first_idx is None):
        raise ValueError("nearest_faces: first_idx for both points and tris or for neither")
    if points_first_idx is None and torch.is_tensor(points):
        points_first_idx = with_host_lengths(torch.zeros((1,), dtype=torch.int64, device=points.device), [0])
        tris_first_idx = with_host_lengths(torch.zeros((1,), dtype=torch.int64, device=points.device), [0])
    pts, tr, seg = _pf_inputs(points, points_first_idx, tris, tris_first_idx, None, min_triangle_area, "nearest_faces")
    d2, idx, _ = _pf_search(0, pts.detach(), tr.detach(), seg, float(min_triangle_area))
    return d2, idx.long()


def _packed_mesh(meshes, fn):
    """(tris (T,3,3), first_idx (N,)) of a Meshes-like object or a (verts (N,V,3), faces (N,F,3) long[, num_faces]) tuple."""
    if all(hasattr(meshes, a) for a in ("verts_packed", "faces_packed", "mesh_to_faces_packed_first_idx",
                                        "num_faces_per_mesh")):
        verts, faces = meshes.verts_packed(), meshes.faces_packed()
        if verts.dim() != 2 or verts.shape[-1] != 3 or faces.dim() != 2 or faces.shape[-1] != 3:
            raise ValueError("%s: verts_packed must be (V, 3) and faces_packed (F, 3)" % fn)
        return verts[faces.long()], meshes.mesh_to_faces_packed_first_idx()
    if not isinstance(meshes, (tuple, list)) or len(meshes) not in (2, 3):
        raise ValueError("%s: meshes must be a Meshes object or a (verts, faces[, num_faces]) tuple" % fn)
    verts, faces = meshes[0], meshes[1]
    if not torch.is_tensor(verts) or verts.dim() != 3 or verts.shape[-1] != 3:
        raise ValueError("%s: verts must be (N, V, 3)" % fn)
    if (not torch.is_tensor(faces) or faces.dim() != 3 or faces.shape[-1] != 3 or faces.shape[0] != verts.shape[0]
            or faces.is_floating_point()):
        raise ValueError("%s: faces must be an integer tensor (N, F, 3) with the batch size of verts" % fn)
    N, F = faces.shape[0], faces.shape[1]
    tris = verts[torch.arange(N, device=verts.device)[:, None, None], faces.long()]          # (N,F,3,3)
    if len(meshes) == 2 or meshes[2] is None:
        num = with_host_lengths(torch.full((N,), F, dtype=torch.int64, device=verts.device), [F] * N)
        return tris.reshape(N * F, 3, 3), _first_of(num, [F] * N)
    num = torch.as_tensor(meshes[2])
    host = host_lengths(num)
    num = num.reshape(-1)
    if len(host) != N or any(l < 0 or l > F for l in host):
        raise ValueError("%s: num_faces must hold one count in [0, %d] per mesh" % (fn, F))
    tris = torch.cat([tris[n, :host[n]] for n in range(N)]) if N else tris.reshape(0, 3, 3)
    return tris, _first_of(num.to(device=verts.device, dtype=torch.int64), host)


def _packed_clouds(pcls, n_meshes, flat_ok, fn):
    """(points (P,3) packed, first_idx (N,) with its host copy) of a padded (N,P,3) tensor or a Pointclouds-like object,
    one cloud per mesh; with flat_ok a (P,3) tensor is one cloud when there is one mesh."""
    if flat_ok and torch.is_tensor(pcls) and pcls.dim() == 2:
        if pcls.shape[-1] != 3 or n_meshes != 1:
            raise ValueError("%s: a (P, 3) tensor is one cloud and needs one mesh, got %s against %d meshes"
                             % (fn, tuple(pcls.shape), n_meshes))
        pcls = pcls[None]
    if flat_ok and torch.is_tensor(pcls) and pcls.dim() != 3:
        raise ValueError("%s: pcls must be (N, P, 3) or (P, 3), got %s" % (fn, tuple(pcls.shape)))
    pts, p_len = convert_pointclouds_to_tensor(pcls)
    if pts.dim() != 3 or pts.shape[-1] != 3:
        raise ValueError("%s: pcls must be (N, P, 3), got %s" % (fn, tuple(pts.shape)))
    N, P = pts.shape[0], pts.shape[1]
    p_len = torch.as_tensor(p_len)
    host = host_lengths(p_len)               # before any view of it: the host copy rides on this very tensor
    p_len = p_len.reshape(-1)
    if len(host) != N or any(l < 0 or l > P for l in host):
        raise ValueError("%s: the clouds' lengths must hold one count in [0, %d] per cloud" % (fn, P))
    if n_meshes != N:
        raise ValueError("%s: meshes and pcls must have the same batch size" % fn)
    if all(l == P for l in host):
        packed = pts.reshape(N * P, 3)
    else:
        packed = torch.cat([pts[n, :host[n]] for n in range(N)])
    return packed, _first_of(p_len.to(device=pts.device, dtype=torch.int64), host)


def point_mesh_face_distance(meshes, pcls, min_triangle_area=0.0):
    """pytorch3d.loss.point_mesh_face_distance: the scalar
    sum_p d2_p / num_points[cloud(p)] / N + sum_t d2_t / num_faces[mesh(t)] / N
    over the points' distances to the nearest face of their mesh and the faces' distances to the nearest point of their
    cloud (point_face_distance, face_point_distance).  `meshes` is an object with verts_packed / faces_packed /
    mesh_to_faces_packed_first_idx / num_faces_per_mesh or a (verts (N,V,3), faces (N,F,3) long[, num_faces]) tuple;
    `pcls` a padded (N,P,3) tensor or a Pointclouds-like object.  The per-cloud and per-mesh sums are added in a fixed
    order: the value and the gradients w.r.t. the points and the triangles are the same bits from run to run (the step from
    the triangles to shared vertices is torch's own indexing backward).  With lengths that carry a host copy (or none) the
    call reads nothing back from the device."""
    fn = "point_mesh_face_distance"
    tris, t_first = _packed_mesh(meshes, fn)
    packed, p_first = _packed_clouds(pcls, t_first.shape[0], False, fn)
    N = t_first.shape[0]
    pts32, tr32, seg = _pf_inputs(packed, p_first, tris, t_first, None, min_triangle_area, fn)
    _, sums_p, _ = _FaceDistance.apply(pts32, tr32, 0, float(min_triangle_area), seg)
    _, sums_t, _ = _FaceDistance.apply(pts32, tr32, 1, float(min_triangle_area), seg)
    point_dist = (sums_p / seg.p_len.clamp(min=1).float()).sum() / float(max(N, 1))
    face_dist = (sums_t / seg.t_len.clamp(min=1).float()).sum() / float(max(N, 1))
    return point_dist + face_dist


# --------------------------------------------------------------------------------------- the sign of the distance to a mesh
_INDEX_LIMIT = 2 ** 31 - 1


def _eps_sqrt(squared, eps=1e-17):
    """DSS/utils/mathHelper.py:20-25: clamp(|x|, eps); the caller takes the root."""
    return squared.abs().clamp_min(eps)


def _packed_mesh_indexed(meshes, fn):
    """_packed_mesh with the indices kept: (verts (V,3), faces (F,3) int64 rows of verts, tris (F,3,3), first_idx (N,)).
    The tuple form's local indices get n * V added; face rows outside [0, V) are the caller's duty (checking them would
    read the device)."""
    tris, first = _packed_mesh(meshes, fn)
    if not isinstance(meshes, (tuple, list)):
        return meshes.verts_packed(), meshes.faces_packed().to(torch.int64), tris, first
    verts, faces = meshes[0], meshes[1]
    N, V, F = verts.shape[0], verts.shape[1], faces.shape[1]
    packed = faces.to(torch.int64) + (torch.arange(N, device=faces.device, dtype=torch.int64) * V)[:, None, None]
    if len(meshes) == 2 or meshes[2] is None:
        packed = packed.reshape(N * F, 3)
    else:
        host = host_lengths(torch.as_tensor(meshes[2]))
        packed = torch.cat([packed[n, :host[n]] for n in range(N)]) if N else packed.reshape(0, 3)
    return verts.reshape(N * V, 3), packed, tris, first


def _pseudonormals(verts, faces):
    """The three vector sets of packed float32 verts (V,3) and int64 faces (F,3) on the GPU."""
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    face_n = torch.empty((F, 3), dtype=torch.float32, device=dev)
    edge_n = torch.empty((F, 3, 3), dtype=torch.float32, device=dev)
    vert_n = torch.empty((V, 3), dtype=torch.float32, device=dev)
    ws_bytes = _lib.load().iso_pfsign_normals_workspace_bytes(V, F)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.call("iso_pfsign_normals", p(verts), p(faces), V, F, p(face_n), p(edge_n), p(vert_n), p(ws), ws_bytes, _lib.stream())
    return face_n, edge_n, vert_n


def _sign_mesh(meshes, fn):
    """Validated (verts f32 (V,3), faces int64 (F,3), tris (F,3,3), first_idx) of a mesh argument; the tensors still where
    the caller has them."""
    verts, faces, tris, first = _packed_mesh_indexed(meshes, fn)
    # the library's own inequalities (iso_pfsign_normals, iso_pfsign_sign): what passes here is not refused there
    if faces.shape[0] >= _INDEX_LIMIT // 3 or verts.shape[0] >= _INDEX_LIMIT:
        raise ValueError("%s: %d vertices and %d faces; the limits are V < 2^31 - 1 and F < (2^31 - 1) / 3"
                         % (fn, verts.shape[0], faces.shape[0]))
    return verts, faces, tris, first


def mesh_pseudonormals(meshes):
    """The angle-weighted pseudonormals of a batch of meshes (Baerentzen & Aanaes), in packed order:
    (face_normals (F,3), edge_normals (F,3,3), vert_normals (V,3)), float32, no gradient.

    face_normals are the unit normals (v1 - v0) x (v2 - v0) / |.|; edge_normals[f, k] belongs to the edge from vertex k
    to vertex k + 1 mod 3 of face f and is the sum of the unit normals of all faces that hold both of its end vertices (one
    face on a boundary, every face of a non-manifold edge); vert_normals[v] is the sum over the corners at v of corner
    angle * face normal.  A face without area has a zero normal and contributes nothing.  Edge and vertex vectors are not
    normalised.  `meshes` as in point_mesh_face_distance; face indices outside the vertices are the caller's duty.  The
    sums run in a fixed order: the same bits from run to run.  A ground-truth mesh does not change between steps: compute
    this once and hand it to point_mesh_sign / point_mesh_signed_distance as `normals`."""
    fn = "mesh_pseudonormals"
    verts, faces, _, _ = _sign_mesh(meshes, fn)
    _on_gpu(verts, faces)
    return _pseudonormals(verts.detach().float().contiguous(), faces.contiguous())


def _sign_normals(normals, verts, faces, fn):
    """The `normals` argument checked against the mesh: three float tensors (F,3), (F,3,3), (V,3)."""
    if not isinstance(normals, (tuple, list)) or len(normals) != 3 or not all(torch.is_tensor(t) for t in normals):
        raise ValueError("%s: normals must be the three tensors mesh_pseudonormals returns" % fn)
    V, F = verts.shape[0], faces.shape[0]
    for t, shape in zip(normals, ((F, 3), (F, 3, 3), (V, 3))):
        if tuple(t.shape) != shape or not t.is_floating_point():
            raise ValueError("%s: normals must be float tensors (F,3), (F,3,3), (V,3) of this mesh, got %s for %s"
                             % (fn, tuple(t.shape), shape))
    return normals


def _sign_inputs(meshes, pcls, min_triangle_area, normals, fn):
    """Everything the two signed calls share, validated before any GPU work."""
    verts, faces, tris, t_first = _sign_mesh(meshes, fn)
    packed, p_first = _packed_clouds(pcls, t_first.shape[0], True, fn)
    if packed.shape[0] >= _INDEX_LIMIT:
        raise ValueError("%s: %d points; the limit is P < 2^31 - 1" % (fn, packed.shape[0]))
    if normals is not None:
        normals = _sign_normals(normals, verts, faces, fn)
    pts32, tr32, seg = _pf_inputs(packed, p_first, tris, t_first, None, min_triangle_area, fn)
    _on_gpu(verts, faces, *(normals or ()))
    return pts32, tr32, seg, verts.detach().float().contiguous(), faces.contiguous(), normals


def _sign_of(points, idx, tris, verts, faces, normals, min_area):
    """sign (P,) f32 and feature (P,) int32 of points whose nearest faces idx (P,) int32 the search has found."""
    if normals is None:
        normals = _pseudonormals(verts, faces)
    face_n, edge_n, vert_n = (t.detach().float().contiguous() for t in normals)
    P, dev = points.shape[0], points.device
    sign = torch.empty((P,), dtype=torch.float32, device=dev)
    feature = torch.empty((P,), dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.call("iso_pfsign_sign", p(points), p(idx), p(tris), p(faces), p(face_n), p(edge_n), p(vert_n), float(min_area),
              p(sign), p(feature), P, faces.shape[0], verts.shape[0], _lib.stream())
    return sign, feature


def point_mesh_sign(meshes, pcls, min_triangle_area=0.0, normals=None, return_parts=False):
    """The sign of the distance from every point to its mesh: (P_total,) float32 in {-1, +1}, packed order, no gradient;
    -1 inside and +1 outside a mesh whose faces are wound outward (reversing the winding reverses the sign).

    The sign is that of (p - c) . N with c the closest point of the mesh (the nearest face of point_face_distance, the
    same min_triangle_area) and N the pseudonormal of the feature c lies on: the face, one of its edges or one of its
    vertices (mesh_pseudonormals; pass its result as `normals` to reuse it).  It needs no closed mesh: an open one is
    signed by the side of its nearest feature.  A point on the mesh, a point whose feature has a zero pseudonormal and a
    point whose mesh has no faces get +1.  With return_parts also (idx (P_total,) int64 into the packed faces, -1 = none,
    feature (P_total,) int32: 0 = face, 1..3 = edge slot + 1, 4..6 = corner + 4, -1 = none).

    `meshes` as in point_mesh_face_distance (face indices outside the vertices are the caller's duty); `pcls` likewise,
    and a (P,3) tensor is one cloud when there is one mesh.  With lengths that carry a host copy (or none) the call reads
    nothing back from the device."""
    fn = "point_mesh_sign"
    pts32, tr32, seg, verts, faces, normals = _sign_inputs(meshes, pcls, min_triangle_area, normals, fn)
    pts32, tr32 = pts32.detach(), tr32.detach()
    _, idx, _ = _pf_search(0, pts32, tr32, seg, float(min_triangle_area))
    sign, feature = _sign_of(pts32, idx, tr32, verts, faces, normals, min_triangle_area)
    return (sign, idx.long(), feature) if return_parts else sign


def point_mesh_signed_distance(meshes, pcls, min_triangle_area=0.0, normals=None):
    """The signed distance from every point to its mesh: (P_total,) float32, packed order:
    point_mesh_sign * sqrt(eps_sqrt(point_face_distance)), which is what the reference's SignedDistanceLoss compares an
    SDF with (DSS/training/losses.py:596), with an exact sign in place of its raster parity.  Differentiable w.r.t. the
    points and the vertices through the distance (point_face_distance's backward pass), the sign and the nearest faces
    held constant.  Arguments as point_mesh_sign."""
    fn = "point_mesh_signed_distance"
    pts32, tr32, seg, verts, faces, normals = _sign_inputs(meshes, pcls, min_triangle_area, normals, fn)
    d2, _, idx = _FaceDistance.apply(pts32, tr32, 0, float(min_triangle_area), seg)
    sign, _ = _sign_of(pts32.detach(), idx, tr32.detach(), verts, faces, normals, min_triangle_area)
    return sign * torch.sqrt(_eps_sqrt(d2))


# ------------------------------------------------------------------- the point regularisers: ProjectionLoss, RepulsionLoss
SurfaceLosses = namedtuple("SurfaceLosses", "projection repulsion normals knn")

_PROJECTION, _REPULSION, _GRADIENTS = 1, 2, 4         # ISO_SURFLOSS_*


class SurfaceKNN(namedtuple("KNN", "dists idx knn")):
    """KNN(dists, idx, knn) of the nearest other points, as pytorch3d names the fields, plus `points`: the detached
    (N,P,3) float32 positions the lists were built on, which stand in for `knn` (N,P,K,3) where that is None."""

    def __new__(cls, dists, idx, knn=None, points=None):
        self = super(SurfaceKNN, cls).__new__(cls, dists, idx, knn)
        self.points = points
        return self


def _rows(t, K):
    """A (N,P,>=K) tensor as the kernels read it: (tensor, row stride).  A [..., 1:] view of a wider result is taken as it
    is; anything else is copied."""
    N, P, st = t.shape[0], t.shape[1], t.stride()
    if t.numel() > 0 and st[2] == 1 and st[1] >= K and (N == 1 or st[0] == P * st[1]):
        return t, st[1]
    t = t.contiguous()
    return t, t.shape[2]


def _rowptr(t):
    """_lib.ptr for a tensor _rows has passed: its rows may be a strided view."""
    if not t.is_cuda:
        raise RuntimeError("iso_points_amd: tensor must live on the GPU (got %s); there is no CPU path" % t.device)
    return ctypes.c_void_p(t.data_ptr())


def _mollify(normals, tree, lengths, filter_scale, inv_sigma2, use_normal_w):
    N, P, _ = normals.shape
    K = tree.idx.shape[2]
    out = torch.empty_like(normals)
    idx, idx_stride = _rows(tree.idx, K)
    dists, d_stride = _rows(tree.dists, K)
    p = _lib.ptr
    _lib.call("iso_surfloss_mollify", p(normals), _rowptr(idx), idx_stride, _rowptr(dists), d_stride, p(lengths),
              N, P, K, float(filter_scale), float(inv_sigma2), int(bool(use_normal_w)), p(out), _lib.stream())
    return out


class _SurfaceSweep(torch.autograd.Function):
    """points -> (projection (N,P) or None, repulsion (N,P) or None).  Everything but `points` is a constant, as in the
    reference (no_grad / detach), so a row's gradient touches its own point only: the forward sweep writes the two
    per-row gradient vectors and the backward pass is a row-wise scale of them."""

    @staticmethod
    def forward(ctx, points, tree, n1, n2, lengths, filter_scale, inv_sigma2, which):
        N, P, _ = points.shape
        K = tree.idx.shape[2]
        dev = points.device
        grad = ctx.needs_input_grad[0]

        def out(flag, *shape):
            return torch.empty(shape, dtype=torch.float32, device=dev) if which & flag else None
        proj, rep = out(_PROJECTION, N, P), out(_REPULSION, N, P)
        g_proj = out(_PROJECTION, N, P, 3) if grad else None
        g_rep = out(_REPULSION, N, P, 3) if grad else None
        idx, idx_stride = _rows(tree.idx, K)
        dists, d_stride = _rows(tree.dists, K)
        knn = tree.knn.detach().float().contiguous() if tree.knn is not None else None
        p = _lib.ptr
        _lib.call("iso_surfloss_forward", p(points), p(tree.points) if knn is None else None, p(knn), p(n1), p(n2),
                  _rowptr(idx), idx_stride, _rowptr(dists), d_stride, p(lengths), N, P, K, float(filter_scale),
                  float(inv_sigma2), which | (_GRADIENTS if grad else 0), p(proj), p(rep), p(g_proj), p(g_rep),
                  _lib.stream())
        ctx.grads = (g_proj, g_rep)
        ctx.set_materialize_grads(False)
        return proj, rep

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, up_proj, up_rep):
        total = None
        for up, g in zip((up_proj, up_rep), ctx.grads):
            if up is None or g is None:
                continue
            term = up.detach().float().unsqueeze(-1) * g
            total = term if total is None else total + term
        return total, None, None, None, None, None, None, None


def _surface_tree(knn, pts, K_asked):
    """A caller's tree checked against the points: SurfaceKNN with float32 dists, int64 idx."""
    if not all(hasattr(knn, a) for a in ("idx", "dists")):
        raise ValueError("surface_losses: knn must carry idx and dists (a KNN of knn_others or pytorch3d's)")
    idx, dists = knn.idx, knn.dists
    nbrs, built_on = getattr(knn, "knn", None), getattr(knn, "points", None)
    if idx.dim() != 3 or tuple(idx.shape[:2]) != tuple(pts.shape[:2]) or tuple(dists.shape) != tuple(idx.shape):
        raise ValueError("surface_losses: knn.idx and knn.dists must be (N, P, K) for points (N, P, 3), got %s and %s for %s"
                         % (tuple(idx.shape), tuple(dists.shape), tuple(pts.shape)))
    if idx.shape[2] < 1 or idx.shape[2] > 32:
        raise ValueError("surface_losses: knn holds %d neighbours per point; the limits are [1, 32]" % idx.shape[2])
    if nbrs is None and built_on is None:
        raise ValueError("surface_losses: knn must carry the neighbours' positions `knn` (N, P, K, 3) or the `points` it "
                         "was built on")
    if nbrs is not None and tuple(nbrs.shape) != tuple(idx.shape) + (3,):
        raise ValueError("surface_losses: knn.knn must be (N, P, K, 3)")
    if nbrs is None and tuple(built_on.shape) != tuple(pts.shape):
        raise ValueError("surface_losses: knn.points must have the shape of points")
    return idx, dists, nbrs, built_on


def surface_losses(points, normals=None, lengths=None, *, knn_k=33, filter_scale=2.0, sharpness_sigma=0.75,
                   projection=True, repulsion=True, knn=None):
    """The two point regularisers of the splatting renderer from one neighbour search and one pair of normal
    mollifications: SurfaceLosses(projection, repulsion, normals, knn).

    projection  (sum L_b,) packed: the squared distance of every point to the plane fitted through its neighbours
                (ProjectionLoss.compute, DSS/training/losses.py:300-403); None when not asked for
    repulsion   (sum L_b,) packed: minus the weighted mean squared distance from the point, moved onto that plane, to its
                neighbours (RepulsionLoss.compute, :425-515); None when not asked for
    normals     (N,P,3) the twice mollified normals n2 (:332, :337-342), rows beyond a cloud's length zero
    knn         the SurfaceKNN used: the one given, or the knn_k - 1 nearest other points of every point with the detached
                points they were found on

    Both losses are differentiable w.r.t. `points`; weights, normals and neighbour positions are constants, as in the
    reference.  `points` / `normals` are padded (N,P,3) tensors with `lengths`, or `points` is an object with
    points_padded() / normals_padded() / num_points_per_cloud().  knn_k in [2, 33] counts the point itself, as the
    reference's does; every cloud needs at least knn_k points.  A `knn` that is given is used with ITS distances and
    neighbour positions (its `knn` (N,P,K,3), else the `points` it carries): a tree of an earlier step stays the tree of
    that step, as the reference's cached knn_tree does.  The Gaussian bandwidth of the repulsion is L_b / 2 per cloud.
    float32 throughout; the same bits from run to run, and a loss is the same bits whether or not the other is computed.
    Clouds with duplicate points are undefined (0 / 0 in the spacing, as in the reference)."""
    fn = "surface_losses"
    if normals is None and hasattr(points, "normals_padded"):
        normals = points.normals_padded()
    pts, conv_len = convert_pointclouds_to_tensor(points)
    if pts.dim() != 3 or pts.shape[-1] != 3:
        raise ValueError("%s: points must be (N, P, 3), got %s" % (fn, tuple(pts.shape)))
    if normals is None or not torch.is_tensor(normals) or tuple(normals.shape) != tuple(pts.shape):
        raise ValueError("%s: normals must have the shape of points, %s" % (fn, tuple(pts.shape)))
    if int(knn_k) != knn_k or not 2 <= knn_k <= 33:
        raise ValueError("%s: knn_k must be in [2, 33] (the point itself and up to 32 others), got %r" % (fn, knn_k))
    if not float(filter_scale) > 0.0 or not float(sharpness_sigma) > 0.0:
        raise ValueError("%s: filter_scale and sharpness_sigma must be positive" % fn)
    if not (projection or repulsion):
        raise ValueError("%s: ask for the projection, the repulsion or both" % fn)
    if lengths is None:
        lengths = conv_len
    lengths = torch.as_tensor(lengths)
    host = host_lengths(lengths)              # before any reshape: the host copy rides on this very tensor
    if len(host) != pts.shape[0]:
        raise ValueError("%s: lengths must have one entry per cloud" % fn)
    if any(l > pts.shape[1] or l < 0 for l in host):
        raise ValueError("%s: lengths must lie in [0, %d]" % (fn, pts.shape[1]))
    K = int(knn_k) - 1
    given = _surface_tree(knn, pts, K) if knn is not None else None
    if given is not None:
        K = given[0].shape[2]
    if any(l < K + 1 for l in host):
        raise ValueError("%s: every cloud needs at least knn_k = %d points (lengths %s): below that the neighbour lists "
                         "have unfilled slots" % (fn, K + 1, host))
    _on_gpu(pts, normals, *([t for t in given if t is not None] if given is not None else []))
    dev = pts.device
    lens = lengths.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    pts32 = pts.float().contiguous()
    if given is None:
        from .point_processing import knn_others
        found = knn_others(pts32.detach(), lens, K=K)
        tree = SurfaceKNN(found.dists, found.idx, None, pts32.detach())
    else:
        idx, dists, nbrs, built_on = given
        tree = SurfaceKNN(dists.detach().float(), idx.to(torch.int64), nbrs,
                          built_on.detach().float().contiguous() if built_on is not None else None)
    inv_sigma2 = 1.0 / (float(sharpness_sigma) * float(sharpness_sigma))
    n0 = normals.detach().float().contiguous()
    n1 = _mollify(n0, tree, lens, filter_scale, inv_sigma2, False)
    n2 = _mollify(n1, tree, lens, filter_scale, inv_sigma2, True)
    which = (_PROJECTION if projection else 0) | (_REPULSION if repulsion else 0)
    proj, rep = _SurfaceSweep.apply(pts32, tree, n1, n2, lens, float(filter_scale), inv_sigma2, which)
    return SurfaceLosses(padded_to_packed(proj, host) if proj is not None else None,
                         padded_to_packed(rep, host) if rep is not None else None, n2, tree)


class _SurfaceLoss(torch.nn.Module):
    """What ProjectionLoss and RepulsionLoss share: the cached neighbour tree, the keyword overrides and the reduction
    (SurfaceLoss / BaseLoss, DSS/training/losses.py:25-62, :149-276)."""
    _which = None
    _rebuild_default = False

    def __init__(self, reduction="mean", knn_k=33, filter_scale=2.0, sharpness_sigma=0.75):
        super(_SurfaceLoss, self).__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Invalid reduction method (%s)" % (reduction,))
        self.reduction = reduction
        self.knn_k = knn_k
        self.filter_scale = filter_scale
        self.sharpness_sigma = sharpness_sigma
        self.knn_tree = None

    def forward(self, point_clouds, points_filters=None, rebuild_knn=None, reduction=None, filter_scale=None,
                sharpness_sigma=None, knn_tree=None):
        """The loss of `point_clouds` (an object with points_padded / normals_padded / num_points_per_cloud, or a
        (points, normals[, lengths]) tuple of padded tensors), reduced.  filter_scale,
        sharpness_sigma and knn_tree replace the module's own from this call on, as the reference's compute() keeps them;
        `reduction` holds for this call.  A cached tree is reused while its idx.shape[:2] matches the points, with the
        distances and neighbour positions of the moment it was built (:312, :325, :368); rebuild_knn searches again.  A
        cloud object with update_normals_ gets the packed mollified normals, as :222 does; tensors are never modified."""
        if points_filters is not None:
            raise NotImplementedError("points_filters: the reference's visibility filter reads an unbound name "
                                      "(DSS/training/losses.py:214) and cannot run; it is not part of this package")
        reduction = reduction or self.reduction
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Invalid reduction method (%s)" % (reduction,))
        if filter_scale is not None:
            self.filter_scale = filter_scale
        if sharpness_sigma is not None:
            self.sharpness_sigma = sharpness_sigma
        if knn_tree is not None:
            self.knn_tree = knn_tree
        if rebuild_knn is None:
            rebuild_knn = self._rebuild_default
        if isinstance(point_clouds, (tuple, list)):
            if len(point_clouds) not in (2, 3):
                raise ValueError("point_clouds: a (points, normals[, lengths]) tuple or a point-cloud object")
            points, normals = point_clouds[0], point_clouds[1]
            lengths = point_clouds[2] if len(point_clouds) == 3 else None
        else:
            points, normals, lengths = point_clouds, None, None
        shape = tuple(convert_pointclouds_to_tensor(points)[0].shape[:2])
        tree = self.knn_tree
        if rebuild_knn or tree is None or tuple(tree.idx.shape[:2]) != shape:
            tree = None
        res = surface_losses(points, normals, lengths, knn_k=self.knn_k, filter_scale=self.filter_scale,
                             sharpness_sigma=self.sharpness_sigma, projection=self._which == "projection",
                             repulsion=self._which == "repulsion", knn=tree)
        self.knn_tree = res.knn
        if hasattr(point_clouds, "update_normals_"):
            host = host_lengths(torch.as_tensor(point_clouds.num_points_per_cloud()))
            point_clouds.update_normals_(padded_to_packed(res.normals, host))
        loss = res.projection if self._which == "projection" else res.repulsion
        if reduction == "sum":
            return loss.sum()
        if reduction == "mean":
            return loss.mean()
        return loss


class ProjectionLoss(_SurfaceLoss):
    """DSS/training/losses.py:282-403: the squared distance of every point to the plane fitted through its neighbours by
    non-linear kernel regression (Oztireli et al.), per point (sum L_b,) before the reduction.  rebuild_knn defaults to
    False: the tree of the first call is kept while the cloud's shape holds."""
    _which = "projection"
    _rebuild_default = False


class RepulsionLoss(_SurfaceLoss):
    """DSS/training/losses.py:406-515: minus the density-weighted mean squared distance from every point, projected onto its
    local plane, to its neighbours.  rebuild_knn defaults to True.  A cached tree follows ProjectionLoss's rule (the
    reference reads knn_tree.shape at :438, which does not exist)."""
    _which = "repulsion"
    _rebuild_default = True


# ------------------------------------------------------------------------------------ the third point regulariser: NormalLoss
class _Padded(object):
    """A (points, lengths) pair in the shape the estimators take a cloud object."""

    def __init__(self, points, lengths):
        self._points, self._lengths = points, lengths

    def points_padded(self):
        return self._points

    def num_points_per_cloud(self):
        return self._lengths


class NormalLoss(torch.nn.Module):
    """DSS/training/losses.py:86-102: 1 - |cos| between every point's normal and the PCA normal of its K-neighbourhood
    (math_helper.estimate_pointcloud_normals), per valid point (sum L_b,) packed before the reduction; the cosine is
    torch.nn.functional.cosine_similarity's, eps = 1e-8.  Gradients reach the normals through torch and the point
    positions through the local-frame kernel's backward (iso_pca_frames_backward: the neighbour index, the eigenvalue
    order and the signs are constants; math_helper.pca_frames states the rules).  neighborhood_size <= 32."""

    def __init__(self, reduction="mean", neighborhood_size=16):
        super(NormalLoss, self).__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Invalid reduction method (%s)" % (reduction,))
        self.reduction = reduction
        self.neighborhood_size = neighborhood_size

    def forward(self, point_clouds, neighborhood_size=None, reduction=None):
        """The loss of `point_clouds`: an object with points_padded / normals_padded / num_points_per_cloud, or a
        (points, normals[, lengths]) tuple of padded tensors.  neighborhood_size and reduction hold for this call."""
        from .math_helper import estimate_pointcloud_normals
        reduction = reduction or self.reduction
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Invalid reduction method (%s)" % (reduction,))
        if neighborhood_size is None:
            neighborhood_size = self.neighborhood_size
        if isinstance(point_clouds, (tuple, list)):
            if len(point_clouds) not in (2, 3):
                raise ValueError("point_clouds: a (points, normals[, lengths]) tuple or a point-cloud object")
            points, normals = point_clouds[0], point_clouds[1]
            lengths = point_clouds[2] if len(point_clouds) == 3 else None
        else:
            points, normals, lengths = point_clouds, None, None
            if hasattr(point_clouds, "normals_padded"):
                normals = point_clouds.normals_padded()
        pts, conv_len = convert_pointclouds_to_tensor(points)
        if pts.dim() != 3 or pts.shape[-1] != 3:
            raise ValueError("NormalLoss: points must be (N, P, 3), got %s" % (tuple(pts.shape),))
        if normals is None or not torch.is_tensor(normals) or tuple(normals.shape) != tuple(pts.shape):
            raise ValueError("NormalLoss: normals must have the shape of points, %s" % (tuple(pts.shape),))
        if lengths is None:
            lengths = conv_len
        lengths = torch.as_tensor(lengths)
        host = host_lengths(lengths)              # before any reshape: the host copy rides on this very tensor
        if len(host) != pts.shape[0] or any(l > pts.shape[1] or l < 0 for l in host):
            raise ValueError("NormalLoss: lengths must hold one count in [0, %d] per cloud" % pts.shape[1])
        _on_gpu(pts, normals)
        lengths = with_host_lengths(lengths.reshape(-1).to(device=pts.device, dtype=torch.int64), host)
        normals_ref = estimate_pointcloud_normals(_Padded(pts, lengths), neighborhood_size=neighborhood_size)
        loss = 1 - torch.nn.functional.cosine_similarity(padded_to_packed(normals, host),
                                                         padded_to_packed(normals_ref, host)).abs()
        if reduction == "sum":
            return loss.sum()
        if reduction == "mean":
            return loss.mean()
        return loss


class NormalLengthLoss(torch.nn.Module):
    """DSS/training/losses.py:74-83: (|n| - 1)^2 per normal, the Eikonal term on the normals of
    sdf_models.get_normals_from_grad(requires_grad=True); plain torch on top of the fused SIREN backward."""

    def __init__(self, reduction="mean", **kwargs):
        super(NormalLengthLoss, self).__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Invalid reduction method (%s)" % (reduction,))
        self.reduction = reduction

    def forward(self, normals, reduction=None):
        reduction = reduction or self.reduction
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("Invalid reduction method (%s)" % (reduction,))
        if normals.shape[-1] != 3:
            raise ValueError("NormalLengthLoss: normals must be (..., 3), got %s" % (tuple(normals.shape),))
        loss = (normals.norm(p=2, dim=-1) - 1) ** 2
        if reduction == "sum":
            return loss.sum()
        if reduction == "mean":
            return loss.mean()
        return loss
