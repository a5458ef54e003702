"""Host-side mirror of the local-frame estimators of DSS/utils/mathHelper.py:

  estimate_pointcloud_local_coord_frames   mathHelper.py:43-119    kNN + per-point PCA (iso_pca_frames)
  estimate_pointcloud_normals              mathHelper.py:122-156   column 0 of those frames

The reference builds them on pytorch3d.ops.knn_points and the CUDA extension torch_batch_svd; here the exact kNN is
point_processing.knn_points and the gather, mean, covariance, eigensolve, ordering and sign rule are one HIP kernel
(csrc/pca.hip).  With grad mode on and points that require grad the frames carry a gradient into the point positions
(iso_pca_frames_backward, csrc/pca_backward.hip), as the reference's do through torch_batch_svd's backward; the neighbour
index, the eigenvalue order, the clamp and the signs are constants.  Limit: neighborhood_size <= 32 (the exact kNN's
selection list).
"""
import torch

from . import _lib
from .levelset_sampling import convert_pointclouds_to_tensor, host_lengths

MAX_NEIGHBORHOOD = 32          # frnn.frnn_grid_points' exact selection list (point_processing.knn_points)


def _refuse_cpu_backward(points):
    """A CPU tensor that asks for a gradient is refused rather than detached silently."""
    if torch.is_grad_enabled() and points.requires_grad and not points.is_cuda:
        raise NotImplementedError("iso_points_amd: the local-frame kernel has its backward on the GPU only; move the points "
                                  "there, or call it under torch.no_grad() or on detached points")


def _check(points, num_points, neighborhood_size):
    """The reference's refusals, then this package's own limits; all before any GPU work."""
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("The pointclouds argument has to be of shape (minibatch, N, 3)")
    lens = host_lengths(num_points) if num_points.is_cuda else [int(x) for x in num_points.tolist()]
    if any(l <= neighborhood_size for l in lens):
        raise ValueError("The neighborhood_size argument has to be >= size of each of the point clouds.")
    if neighborhood_size > MAX_NEIGHBORHOOD:
        raise NotImplementedError("iso_points_amd: neighborhood_size %d > %d: the exact kNN (point_processing.knn_points) "
                                  "keeps at most %d neighbours" % (neighborhood_size, MAX_NEIGHBORHOOD, MAX_NEIGHBORHOOD))
    if neighborhood_size < 1:
        raise ValueError("neighborhood_size must be >= 1")
    _refuse_cpu_backward(points)
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")


def _frames_forward(pts, lens, ids, disambiguate):
    """iso_pca_frames on float32 contiguous points, int64 lengths and index: (curvature, frames)."""
    N, P, _ = pts.shape
    K = ids.shape[2]
    curv = torch.empty((N, P, 3), dtype=torch.float32, device=pts.device)
    frames = torch.empty((N, P, 3, 3), dtype=torch.float32, device=pts.device)
    work = None
    if disambiguate:
        work = torch.empty((max(_lib.load().iso_pca_frames_work_bytes(N), 1),), dtype=torch.uint8, device=pts.device)
    _lib.call("iso_pca_frames", _lib.ptr(pts), _lib.ptr(lens), _lib.ptr(ids), N, P, K, 1 if disambiguate else 0,
              _lib.ptr(work), _lib.ptr(curv), _lib.ptr(frames), _lib.stream())
    return curv, frames


class _PcaFrames(torch.autograd.Function):
    """points -> (curvature, frames): iso_pca_frames, and iso_pca_frames_backward on the forward's own outputs.  The index,
    the eigenvalue order, the clamp and the signs are constants of the backward."""

    @staticmethod
    def forward(ctx, pts, lens, ids, disambiguate):
        curv, frames = _frames_forward(pts, lens, ids, disambiguate)
        ctx.save_for_backward(pts, lens, ids, curv, frames)
        ctx.disambiguate = disambiguate
        ctx.set_materialize_grads(False)
        return curv, frames

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_curv, g_frames):
        pts, lens, ids, curv, frames = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_curv is None and g_frames is None):
            return None, None, None, None
        N, P, _ = pts.shape
        K = ids.shape[2]
        grad = torch.empty_like(pts)
        if grad.numel() == 0:
            return grad, None, None, None

        def f32(g):
            return g.detach().float().contiguous() if g is not None else None
        g_curv, g_frames = f32(g_curv), f32(g_frames)
        ws_bytes = _lib.load().iso_pca_frames_backward_work_bytes(N, P, K)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=pts.device)
        p = _lib.ptr
        _lib.call("iso_pca_frames_backward", p(pts), p(lens), p(ids), N, P, K, 1 if ctx.disambiguate else 0, p(curv),
                  p(frames), p(g_curv), p(g_frames), p(ws), ws_bytes, p(grad), _lib.stream())
        return grad, None, None, None


def pca_frames(points, num_points, idx, disambiguate_directions=True):
    """iso_pca_frames on a padded cloud (N,P,3), lengths (N,) and the (N,P,K) int64 kNN index (the point itself included).
    Returns (curvature (N,P,3) ascending, frames (N,P,3,3), eigenvector c in column c); padded rows are zero.

    With grad mode on and points that require grad both results are differentiable w.r.t. the points, with everything
    the forward decides discretely held constant: the index rows, the ascending order, the clamp at 0 and the signs.  The
    forward's launches and bits are the same either way.  Where the eigen adjoint is undefined this package rules: an
    eigenvalue pair closer than 2e-5 lambda_max (the tolerance the forward's eigenvalues are judged by) exchanges nothing,
    where torch's eigh backward gives inf / NaN; a row of K exact duplicates (lambda_max = 0) has a zero gradient; an
    eigenvalue that is 0 (clamped) passes none; padded rows give and receive nothing, whatever the incoming gradients
    hold there.  float32 throughout; no float atomics: two backward runs give the same bits."""
    lens = num_points.to(device=points.device, dtype=torch.int64).contiguous()
    ids = idx.to(torch.int64).contiguous()
    _refuse_cpu_backward(points)
    if torch.is_grad_enabled() and points.requires_grad:
        return _PcaFrames.apply(points.float().contiguous(), lens, ids, bool(disambiguate_directions))
    return _frames_forward(points.detach().float().contiguous(), lens, ids, bool(disambiguate_directions))


def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=50, disambiguate_directions=True,
                                           return_knn_result=False):
    """Principal directions of the K-neighbourhood of every point (mathHelper.py:43-119).

    pointclouds: padded tensor (N,P,3) or an object with points_padded() / num_points_per_cloud().
    Returns (curvature (N,P,3), frames (N,P,3,3)) [+ knn_result]: eigenvalues of the neighbourhood covariance
    (1/K) sum (x_j - m)(x_j - m)^T (= S^2 / K of the reference's SVD) in ascending order, and frames[..., :, c] the c-th
    principal direction (column 0 = normal).  With disambiguate_directions the reference's sign rule is applied to columns
    0 and 2 (tested against the globally centred point, as the reference does) and column 1 = col0 x col2.
    Padded rows (i >= num_points[b]) are zero.

    neighborhood_size must be <= 32 (the exact kNN's limit); the default of 50 is kept for signature parity and raises
    NotImplementedError -- every caller in the reference passes 8, 12, 16 or 31.

    With grad mode on and GPU points that require grad, curvature and frames are differentiable w.r.t. the points
    (pca_frames states the rules: the neighbour index, the order, the clamp and the signs are constants; near-equal
    eigenvalues exchange nothing; duplicates and padded rows give zero).  The forward's bits do not depend on it.  The kNN
    tuple of return_knn_result stays what knn_points returns and carries no graph.  The backward exists on the GPU only:
    a CPU tensor that requires grad raises NotImplementedError rather than detaching silently.
    """
    from .point_processing import knn_points
    points, num_points = convert_pointclouds_to_tensor(pointclouds)
    _check(points, num_points, neighborhood_size)
    knn_result = knn_points(points, points, num_points, num_points, K=neighborhood_size, return_nn=return_knn_result)
    curvature, frames = pca_frames(points, num_points, knn_result.idx, disambiguate_directions)
    if return_knn_result:
        return curvature, frames, knn_result
    return curvature, frames


def estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True):
    """Normals = column 0 of estimate_pointcloud_local_coord_frames (mathHelper.py:122-156), (N,P,3); same limits, and
    differentiable w.r.t. the points under the same rules."""
    _, frames = estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=neighborhood_size,
                                                       disambiguate_directions=disambiguate_directions)
    return frames[:, :, :, 0]
