"""Host-side mirror of the local-frame estimators of DSS/utils/mathHelper.py:

  estimate_pointcloud_local_coord_frames   mathHelper.py:43-119    kNN + per-point PCA (iso_pca_frames)
  estimate_pointcloud_normals              mathHelper.py:122-156   column 0 of those frames

The reference builds them on pytorch3d.ops.knn_points and the CUDA extension torch_batch_svd; here the exact kNN is
point_processing.knn_points and the gather, mean, covariance, eigensolve, ordering and sign rule are one HIP kernel
(csrc/pca.hip).  Limits: neighborhood_size <= 32 (the exact kNN's selection list) and no backward.
"""
import torch

from . import _lib
from .levelset_sampling import convert_pointclouds_to_tensor, host_lengths

MAX_NEIGHBORHOOD = 32          # frnn.frnn_grid_points' exact selection list (point_processing.knn_points)


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
    if torch.is_grad_enabled() and points.requires_grad:
        raise NotImplementedError("iso_points_amd: the local-frame kernel has no backward; call it under torch.no_grad() "
                                  "or on detached points")
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")


def pca_frames(points, num_points, idx, disambiguate_directions=True):
    """iso_pca_frames on a padded cloud (N,P,3), lengths (N,) and the (N,P,K) int64 kNN index (the point itself included).
    Returns (curvature (N,P,3) ascending, frames (N,P,3,3), eigenvector c in column c); padded rows are zero."""
    N, P, _ = points.shape
    K = idx.shape[2]
    pts = points.detach().float().contiguous()
    lens = num_points.to(device=pts.device, dtype=torch.int64).contiguous()
    ids = idx.to(torch.int64).contiguous()
    curv = torch.empty((N, P, 3), dtype=torch.float32, device=pts.device)
    frames = torch.empty((N, P, 3, 3), dtype=torch.float32, device=pts.device)
    work = None
    if disambiguate_directions:
        work = torch.empty((max(_lib.load().iso_pca_frames_work_bytes(N), 1),), dtype=torch.uint8, device=pts.device)
    _lib.call("iso_pca_frames", _lib.ptr(pts), _lib.ptr(lens), _lib.ptr(ids), N, P, K, 1 if disambiguate_directions else 0,
              _lib.ptr(work), _lib.ptr(curv), _lib.ptr(frames), _lib.stream())
    return curv, frames


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
    NotImplementedError -- every caller in the reference passes 8, 12, 16 or 31.  There is no backward: grad mode with
    points that require grad raises NotImplementedError rather than detaching silently.
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
    """Normals = column 0 of estimate_pointcloud_local_coord_frames (mathHelper.py:122-156), (N,P,3); same limits."""
    _, frames = estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=neighborhood_size,
                                                       disambiguate_directions=disambiguate_directions)
    return frames[:, :, :, 0]
