"""Chamfer distance between point clouds: pytorch3d.loss.chamfer_distance as the reference calls it
(evaluation.py:119-122 and :169-172 -- chamfer_p / chamfer_n; DSS/training/trainer.py:256 -- the validation
metric train_mvr.py:196 selects checkpoints by).

The nearest-point search runs on the cell grid of iso_points_amd.frnn (exact, any distance), fused with the
normal term and the per-cloud sums; the backward pass is a gather over counting-sorted index lists.  Neither
uses float atomics: values and gradients are the same bits from run to run (include/isopoints.h section G).
"""
import torch

from . import _lib
from . import frnn
from .levelset_sampling import convert_pointclouds_to_tensor

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
    if lengths.dim() != 1:
        lengths = lengths.reshape(-1)
    if lengths.shape[0] != pts.shape[0]:
        raise ValueError("chamfer_distance: %s_lengths must have one entry per cloud" % what)
    # the range check reads the lengths on the host: the host copy where the tensor carries one (full_lengths and every
    # lengths tensor this package returns), so that only lengths built by the caller on the GPU cost a device read
    host = getattr(lengths, "_iso_host", None)
    if host is None or getattr(lengths, "_iso_host_version", None) != lengths._version:
        host = lengths.tolist()
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
