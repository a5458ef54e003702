"""Host-side mirror of the iso-point parts of DSS/utils/point_processing.py
(SURVEY 8(a) rows a8/a9 and 8(f)):

  upsample            point_processing.py:281-362   sparsest-edge midpoint insertion
  wlop                point_processing.py:35-122    FPS subsample + 3 LOP iterations
  farthest_sampling   point_processing.py:473-499   (torch_cluster.fps)
  knn_points          pytorch3d.ops.knn_points as upsample uses it (:315,:358)
  knn_others          the K nearest other points: knn_points(K + 1)[..., 1:] without the slot of the point itself
  denoise_normals     point_processing.py:241-278   bilateral normal filter on the FRNN neighbourhood
  remove_outliers     point_processing.py:16-31     drop points whose neighbourhood is not flat (math_helper)
  remove_close        Poisson-disk elimination: the step behind trimesh's sample_surface_even (config.py:227,
                      DSS/training/trainer.py:255) and pcu.sample_mesh_poisson_disk (DSS/utils/dataset.py:123)

Inputs are padded tensors (N,P,3) + lengths (pytorch3d's Pointclouds container is out of scope;
objects exposing points_padded()/num_points_per_cloud() are accepted).  Neighbour search, the
K^2 sparsity scan and FPS run in libisopoints_hip.so; the remaining glue is a handful of torch
ops on the GPU, exactly where the reference has them.
"""
import math
from collections import namedtuple

import torch

from . import _lib
from . import frnn
from .levelset_sampling import (cloud_diag, convert_pointclouds_to_tensor, eps_denom, full_lengths, host_lengths,
                                with_host_lengths)

_KNN = namedtuple("KNN", "dists idx knn")


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, return_nn=False, return_sorted=True):
    """Exact K nearest neighbours (squared distances, ascending; ties -> lower index).
    Implemented as the FRNN ring search with an infinite radius.  Like pytorch3d, slots that
    cannot be filled (cloud 2 has fewer than K points) hold idx 0 / dist 0."""
    N = p1.shape[0]
    r = torch.full((N,), float("inf"), dtype=torch.float32, device=p2.device)
    # cells sized so that the K-th neighbour is (mostly) closer than one cell: the query then ends
    # in its 3x3x3 fast path instead of the ring walk (same result for any cell size)
    l2 = frnn._as_lengths(lengths2, N, p2.shape[1], p2.device)
    grid = frnn.build_grid(p2.detach().float().contiguous(), l2, r, points_per_cell=max(8.0, 0.75 * K))   # measured optimum (tools/ear_bench.py)
    dists, idxs, nn, _ = frnn.frnn_grid_points(p1, p2, lengths1, lengths2, K=K, r=r, grid=grid,
                                               return_nn=return_nn)
    pad = idxs < 0
    dists = torch.where(pad, torch.zeros_like(dists), dists)
    idxs = torch.where(pad, torch.zeros_like(idxs), idxs)
    if nn is not None:
        nn = nn  # frnn already zero-fills the padded rows
    return _KNN(dists=dists, idx=idxs, knn=nn)


def knn_others(points, lengths=None, K=32, return_nn=False):
    """The K nearest OTHER points of every point of its own cloud: KNN(dists (N,P,K) squared / ascending, idx (N,P,K) int64,
    knn (N,P,K,3) or None), the query's own row left out (iso_frnn_query_others).  On a cloud without duplicate points this
    is knn_points(points, points, K=K + 1)[..., 1:], the "self plus K" search of the reference's losses
    (DSS/training/losses.py:169-180), so K = 32 serves its default knn_k = 33 with the 32-slot list.  Infinite radius, the
    grid knn_points builds; slots that cannot be filled (a cloud of fewer than K + 1 points) and rows beyond `lengths` hold
    idx 0 / dist 0, like pytorch3d.  With duplicate points a duplicate is a neighbour at distance 0."""
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("knn_others: points must be (N, P, 3), got %s" % (tuple(points.shape),))
    if K < 1 or K > 32:
        raise ValueError("K must be in [1, 32], got %d" % K)
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
    N, P, _ = points.shape
    dev = points.device
    pts = points.detach().float().contiguous()
    r = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    lens = frnn._as_lengths(lengths, N, P, dev)
    dists = torch.zeros((N, P, K), dtype=torch.float32, device=dev)
    idxs = torch.zeros((N, P, K), dtype=torch.int64, device=dev)
    nn = torch.zeros((N, P, K, 3), dtype=torch.float32, device=dev) if return_nn else None
    if N > 0 and P > 0:
        grid = frnn.build_grid(pts, lens, r, points_per_cell=max(8.0, 0.75 * (K + 1)))    # as knn_points(K + 1)
        p = _lib.ptr
        ws_bytes = _lib.load().iso_frnn_query_workspace_bytes(N, P, P)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        _lib.call("iso_frnn_query_others", p(pts), p(grid.sorted_points), p(grid.sorted_idx), p(lens), p(grid.off),
                  p(grid.params), p(r), K, p(dists), p(idxs), p(nn), N, P, grid.g_stride, p(ws), ws_bytes, _lib.stream())
        pad = idxs < 0
        dists.masked_fill_(pad, 0.0)
        idxs.masked_fill_(pad, 0)
    return _KNN(dists=dists, idx=idxs, knn=nn)


def _upsample_candidates(points, knn):
    """(N,P,3), (N,P,K,3) -> sparsity (N,P), candidate (N,P,3)  [point_processing.py:326-339]."""
    N, P, K = knn.shape[0], knn.shape[1], knn.shape[2]
    pts = points.detach().float().contiguous()
    kn = knn.detach().float().contiguous()
    spars = torch.empty((N, P), dtype=torch.float32, device=pts.device)
    cand = torch.empty((N, P, 3), dtype=torch.float32, device=pts.device)
    _lib.call("iso_upsample_candidates", _lib.ptr(pts), _lib.ptr(kn), N * P, K, _lib.ptr(spars), _lib.ptr(cand),
              _lib.stream())
    return spars, cand


def upsample(pcl, n_points, num_points=None, neighborhood_size=16, knn_result=None):
    """Iteratively add midpoints in the sparsest regions until every cloud has n_points
    (point_processing.py:281-362).  Returns (points_padded, num_points)."""
    points, np_conv = convert_pointclouds_to_tensor(pcl)
    if num_points is None:
        num_points = np_conv
    knn_k = neighborhood_size
    dev = points.device
    if not torch.is_tensor(n_points):
        n_points = torch.full_like(num_points, int(n_points))
    n_points = n_points.to(dev)
    if int(num_points.sum()) == 0:
        return points, num_points
    n_remaining = (n_points - num_points).to(dtype=torch.long)
    if bool((n_remaining <= 0).all()):
        return points, num_points

    def _knn(pts, lens):
        r = knn_points(pts, pts, lens, lens, K=knn_k + 1, return_nn=True, return_sorted=True)
        return _KNN(dists=r.dists[..., 1:], idx=r.idx[..., 1:], knn=r.knn[..., 1:, :])

    if knn_result is None:
        knn_result = _knn(points, num_points)
    while True:
        if bool((n_remaining == 0).all()):
            break
        batch_size, P, _ = points.shape
        max_P = P // 8
        father_sparsity, cand = _upsample_candidates(points, knn_result.knn)            # :331-339
        sparsity_sorted = father_sparsity.sort(dim=1).indices
        n_new_points = n_remaining.clone()
        n_new_points[n_new_points > max_P] = max_P
        sparsity_sorted = sparsity_sorted[:, -max_P:] if max_P > 0 else sparsity_sorted[:, :0]
        new_pts = torch.gather(cand, 1, sparsity_sorted.unsqueeze(-1).expand(-1, -1, 3))
        lens = [int(x) for x in num_points.tolist()]
        nnew = [int(x) for x in n_new_points.tolist()]
        total = []
        for b in range(batch_size):
            # reference quirk kept on purpose: `new_pts[b][-n:]` with n == 0 is the WHOLE array
            # (point_processing.py:352), so a cloud that is already full in a heterogeneous batch
            # still gets max_P rows prepended (the reference warns about such batches, :305-307)
            nb = new_pts[b][new_pts.shape[1] - nnew[b]:] if nnew[b] > 0 else new_pts[b]
            total.append(torch.cat([nb, points[b, :lens[b]]], dim=0))                    # :350-353
        mx = max(t.shape[0] for t in total)
        points = points.new_zeros((batch_size, mx, 3))
        for b, t in enumerate(total):
            points[b, : t.shape[0]] = t
        n_remaining = n_remaining - n_new_points
        num_points = n_new_points + num_points
        if max_P == 0:
            break
        knn_result = _knn(points, num_points)
    return points, num_points


# ----------------------------------------------------------------------------- FPS / WLOP
def farthest_sampling(points, num_points, ratio, random_start=False, generator=None):
    """Farthest-point sampling of ceil(ratio * n) points per cloud (torch_cluster.fps semantics;
    point_processing.py:473-499).  points (N,P,3) padded.  Returns (sampled_padded, num_sampled,
    idx_padded).  random_start=False starts from point 0 of each cloud (deterministic); True draws
    the start like torch_cluster does."""
    N, P, _ = points.shape
    dev = points.device
    lens = host_lengths(num_points)
    ns = [int(math.ceil(ratio * l)) for l in lens]
    mx = max(ns) if ns else 0
    pts = points.detach().float().contiguous()
    start = torch.zeros((N,), dtype=torch.int64, device=dev)
    if random_start:
        u = torch.rand((N,), generator=generator, device="cpu")
        start = (u * torch.tensor(lens, dtype=torch.float32)).long().clamp(max=max(max(lens) - 1, 0)).to(dev)
    out_idx = torch.full((N, max(mx, 1)), -1, dtype=torch.int64, device=dev)
    nsamp = with_host_lengths(torch.tensor(ns, dtype=torch.int64, device=dev), ns)
    work = torch.empty((_lib.load().iso_farthest_point_sampling_work_floats(N, P),), dtype=torch.float32, device=dev)
    if mx > 0:
        _lib.call("iso_farthest_point_sampling", _lib.ptr(pts), _lib.ptr(num_points.to(torch.int64).contiguous()),
                  _lib.ptr(nsamp), _lib.ptr(start), N, P, out_idx.shape[1], _lib.ptr(work), _lib.ptr(out_idx),
                  _lib.stream())
    safe = out_idx.clamp(min=0)
    sampled = torch.gather(pts, 1, safe.unsqueeze(-1).expand(-1, -1, 3))
    sampled = sampled * (out_idx >= 0).unsqueeze(-1).float()
    return sampled[:, :mx], nsamp, out_idx[:, :mx]


def wlop(points, num_points=None, ratio=0.5, neighborhood_size=16, iters=3, repulsion_mu=0.5,
         generator=None, perturb=True, random_start=False):
    """Weighted locally optimal projection (point_processing.py:35-122) on padded tensors.
    Returns (X (N,I,3), num_points_X).  `perturb` adds the reference's randn*h*0.1 offset (:59)."""
    P, num_P = convert_pointclouds_to_tensor(points)
    if num_points is not None:
        num_P = num_points
    dev = P.device
    lensP = host_lengths(num_P)
    N = P.shape[0]
    # bbox diagonal per cloud over the valid points (Pointclouds.get_bounding_boxes, :43-45)
    diag = cloud_diag(P, num_P.to(torch.int64).contiguous())
    h = 4 * torch.sqrt(diag / num_P.float())
    search_radius = torch.clamp(h * neighborhood_size, max=0.2)          # min(h*ns, 0.2) per cloud (:47)
    theta_sigma_inv = 16 / h / h
    if ratio < 1.0:
        X, num_X, _ = farthest_sampling(P, num_P, ratio, random_start=random_start, generator=generator)
    elif ratio == 1.0:
        X, num_X = P.clone(), num_P
    else:
        raise ValueError("ratio must be less or equal to 1.0")
    if perturb:
        noise = torch.randn(X.shape, generator=generator, device="cpu").to(dev) if generator is not None \
            else torch.randn_like(X)
        X = X + noise * (h * 0.1).view(-1, 1, 1)
    falloff = theta_sigma_inv.view(-1, 1, 1)

    def weight(r2, ids):                       # theta(r) = exp(-16 r^2 / h^2), zero for a missing neighbour
        return torch.exp(-r2 * falloff).masked_fill(ids < 0, 0.0)

    K = neighborhood_size
    _, ids_pp, _, grid = frnn.frnn_grid_points(P, P, num_P, num_P, K=K + 1, r=search_radius)
    ids_pp = ids_pp[..., 1:].contiguous()
    gap_pp = torch.norm(P.unsqueeze(-2) - frnn.frnn_gather(P, ids_pp), dim=-1)
    dens_P = weight(gap_pp ** 2, ids_pp).sum(dim=-1) + 1                    # local density of the input cloud (:66-70)
    for _ in range(iters):
        _, ids_xp, _, grid = frnn.frnn_grid_points(X, P, num_X, num_P, K=K, r=search_radius, grid=grid)
        _, ids_xx, _, _ = frnn.frnn_grid_points(X, X, num_X, num_X, K=K + 1, r=search_radius)
        ids_xx = ids_xx[..., 1:].contiguous()
        anchor = frnn.frnn_gather(P, ids_xp)                                 # input points near each sample
        to_anchor = X.unsqueeze(-2) - anchor
        to_peer = X.unsqueeze(-2) - frnn.frnn_gather(X, ids_xx)
        r2_anchor, r2_peer = (to_anchor ** 2).sum(dim=-1), (to_peer ** 2).sum(dim=-1)
        dens_X = torch.exp(-r2_peer * falloff).sum(dim=-1) + 1
        # attraction to the input, each anchor discounted by its density; repulsion among the samples (:84-118)
        pull = weight(r2_anchor, ids_xp) / eps_denom(to_anchor.norm(dim=-1)) / \
            frnn.frnn_gather(dens_P.unsqueeze(-1), ids_xp).squeeze(-1)
        pull = pull.masked_fill(ids_xp < 0, 0.0)
        push = dens_X.unsqueeze(-1) * (torch.exp(-r2_peer * falloff) / eps_denom(to_peer.norm(dim=-1)))
        push = push.masked_fill(ids_xx < 0, 0.0)
        X = (pull[..., None] * anchor).sum(dim=-2) / eps_denom(pull.sum(dim=-1, keepdim=True)) + \
            repulsion_mu * (push[..., None] * to_peer).sum(dim=-2) / eps_denom(push.sum(dim=-1, keepdim=True))
    return X, num_X


def resample_uniformly(points, num_points=None, neighborhood_size=8, shrink_ratio=0.5, repulsion_mu=1.0,
                       generator=None):
    """wlop + upsample back to the original count (point_processing.py:126-166, tensor inputs)."""
    pts, num = convert_pointclouds_to_tensor(points)
    if num_points is not None:
        num = num_points
    X, num_X = wlop(pts, num, ratio=shrink_ratio, repulsion_mu=repulsion_mu, generator=generator)
    return upsample(X, num, num_points=num_X)


def denoise_normals(points, normals, sharpness_sigma=30, knn_result=None, neighborhood_size=16):
    """Bilateral normal filter (point_processing.py:241-278), one cloud: weights
    exp(-((1 - <n, n_i>) / sharpness_sigma)^2) exp(-|p - p_i|^2 P/2) cut at |p - p_i|^2 > 32/P, over
    the FRNN neighbourhood of radius min(4 sqrt(diag/P) K, 0.2).  `sharpness_sigma` divides as given
    (the reference does not convert the angle here, :263).  A `knn_result` must carry idx (and dists);
    its `knn` is gathered when missing (the reference's own branch for a given `knn` reads an
    unbound local, :269)."""
    points, num_points = convert_pointclouds_to_tensor(points)
    if not points.is_cuda:
        raise RuntimeError("iso_points_amd: points must be on the GPU; there is no CPU path")
    if points.shape[0] != 1:
        raise NotImplementedError("denoise_normals: one cloud per call (math.sqrt(diag / P) at :249 "
                                  "needs a single-element tensor)")
    unit = torch.nn.functional.normalize(normals, dim=-1)
    if knn_result is None:
        extent = (points.amax(dim=-2) - points.amin(dim=-2)).norm(dim=-1)
        radius = min(4 * neighborhood_size * math.sqrt(extent / points.shape[1]), 0.2)
        d2, ids, _, _ = frnn.frnn_grid_points(points, points, num_points, num_points, K=neighborhood_size + 1, r=radius,
                                              grid=None, return_nn=True)
        knn_result = _KNN(dists=d2[..., 1:], idx=ids[..., 1:], knn=None)
    nbr_p = knn_result.knn if knn_result.knn is not None else frnn.frnn_gather(points, knn_result.idx, num_points)
    nbr_n = frnn.frnn_gather(unit, knn_result.idx, num_points)
    bandwidth = num_points / 2.0                                      # 1 / sigma_p^2 = P / 2
    gap2 = (nbr_p - points[:, :, None, :]).square().sum(dim=-1)
    w = torch.exp(-gap2 * bandwidth).masked_fill(gap2 > 16 / bandwidth, 0.0) * \
        torch.exp(-(((1 - (nbr_n * unit[:, :, None, :]).sum(dim=-1)) / sharpness_sigma) ** 2))
    mean = (nbr_n * w[..., None]).sum(dim=-2) / eps_denom(w.sum(dim=-1, keepdim=True))
    return torch.nn.functional.normalize(mean, dim=-1).view_as(normals)


def remove_outliers(pointclouds, neighborhood_size=16, tolerance=0.05):
    """Keep the points whose K-neighbourhood is flat: lambda0 / (lambda0 + lambda1 + lambda2) < tolerance over the
    ascending covariance eigenvalues of math_helper.estimate_pointcloud_local_coord_frames, and that lie inside their
    cloud's length (point_processing.py:16-31).  Returns the kept points compacted per cloud, in order, as
    (points_padded (N, max kept, 3), num_points (N,)), the way upsample / wlop return.  The ratio is the reference's plain
    division: in a neighbourhood of exact duplicates it is 0 / 0 = NaN and the point is dropped, as in the reference.
    Same limit as the estimator: neighborhood_size <= 32.  The mask is a selection and is computed under no_grad, so points
    that require grad build no graph for it; the kept rows are an ordinary index of `points`."""
    from .math_helper import estimate_pointcloud_local_coord_frames
    points, num_points = convert_pointclouds_to_tensor(pointclouds)
    # only the eigenvalues are read: the sign rule does not change them
    with torch.no_grad():
        variance, _ = estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=neighborhood_size,
                                                             disambiguate_directions=False)
    N, P = points.shape[0], points.shape[1]
    inside = torch.arange(P, device=points.device)[None, :] < num_points.to(points.device)[:, None]
    mask = (variance[..., 0] / torch.sum(variance, dim=-1) < tolerance) & inside
    kept = [int(x) for x in mask.sum(dim=1).tolist()]
    out = points.new_zeros((N, max(kept) if kept else 0, 3))
    for b in range(N):
        out[b, : kept[b]] = points[b][mask[b]]
    return out, with_host_lengths(torch.tensor(kept, dtype=torch.int64, device=points.device), kept)


# rounds of the elimination enqueued between two reads of the number of samples left open: twice the most rounds seen on
# surface samplings at the default radius (5-8 for 900 to 90 000 samples).  A speed knob only: the result does not depend
# on it.
ROUNDS_PER_BATCH = 16

_INDEX_LIMIT = 2 ** 31 - 1


class _NotOnGpu(RuntimeError, ValueError):
    """remove_close's refusal of CPU tensors: the RuntimeError the rest of the package raises, and a ValueError as every
    other bad argument of that function."""


def _eliminate(points, lengths, radius, valid, s_out):
    """The elimination of include/isopoints.h section L on float32 contiguous GPU points (N,P,3), int64 lengths (N,), float32
    radius (N,) and a uint8 mask (N,P) or None: (mask (N,P) uint8, sel (N,s_out) int32, kept (N,) int64, rounds enqueued).
    One read of 4 bytes per ROUNDS_PER_BATCH rounds."""
    N, P, dev = points.shape[0], points.shape[1], points.device
    mask = torch.zeros((N, P), dtype=torch.uint8, device=dev)
    sel = torch.full((N, s_out), -1, dtype=torch.int32, device=dev)
    kept = torch.zeros((N,), dtype=torch.int64, device=dev)
    if N == 0 or P == 0:
        return mask, sel, kept, 0
    grid = frnn.build_grid(points, lengths, radius)
    ws_bytes = _lib.load().iso_disk_workspace_bytes(N, P)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    left = torch.empty((1,), dtype=torch.int32, device=dev)
    p, s = _lib.ptr, _lib.stream()
    _lib.call("iso_disk_begin", p(grid.sorted_points), p(grid.sorted_idx), p(lengths), p(valid), N, P, p(ws), ws_bytes, s)
    batch, done = max(1, int(ROUNDS_PER_BATCH)), 0
    while True:
        _lib.call("iso_disk_rounds", p(lengths), p(grid.off), p(grid.params), p(radius), N, P, grid.g_stride, done, batch,
                  p(left), p(ws), ws_bytes, s)
        done += batch
        if int(left.item()) == 0:
            break
    _lib.call("iso_disk_select", N, P, s_out, p(mask), p(sel), p(kept), p(ws), ws_bytes, s)
    return mask, sel, kept, done


def remove_close(points, radius, lengths=None, valid=None):
    """Poisson-disk elimination: drop points of each cloud until no two that are left are within `radius` of each other, the
    step behind trimesh.sample.sample_surface_even (config.py:227, DSS/training/trainer.py:255) and
    pcu.sample_mesh_poisson_disk (DSS/utils/dataset.py:123) -- by an exact rule of its own, not bit for bit theirs.

    Two points conflict iff d2 <= r2, d2 = (dx*dx + dy*dy) + dz*dz and r2 = r * r in float32.  Point s is kept iff no kept
    point of lower index conflicts with it (serial dart throwing in index order); points beyond `lengths` or with
    valid == 0 are removed and block nobody.  So the kept set of the first k points does not depend on the points after
    them, and the result does not depend on a launch shape, on timing or on ROUNDS_PER_BATCH.

    points (N,P,3) or an object with points_padded() (and num_points_per_cloud(), taken for `lengths` when none are given);
    radius a positive finite float or an (N,) tensor; lengths (N,) integer in [0, P]; valid (N,P), nonzero = take part.
    Returns (mask (N,P) bool, sel (N,P) int64: the kept indices of each cloud in ascending order, -1 beyond, kept (N,)
    int64).  No gradient: the result is integer.

    Host reads: the rounds run in batches of ROUNDS_PER_BATCH launches and the number of points still undecided (4 bytes)
    is read after each batch; surface samplings finish inside the first batch, so a call normally reads 4 bytes back once
    (a chain of n points, each removing the next, needs n rounds).  `lengths` on the device without a host copy cost one
    more read for the range check."""
    fn = "remove_close"
    if not torch.is_tensor(points):
        if not hasattr(points, "points_padded"):
            raise ValueError("%s: points must be a (N, P, 3) tensor or an object with points_padded()" % fn)
        if lengths is None and hasattr(points, "num_points_per_cloud"):
            lengths = points.num_points_per_cloud()
        points = points.points_padded()
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("%s: points must be (N, P, 3)" % fn)
    N, P = points.shape[0], points.shape[1]
    if torch.is_tensor(radius):
        if radius.dim() != 1 or radius.shape[0] != N:
            raise ValueError("%s: a radius tensor must be of shape (N,)" % fn)
    else:
        try:
            radius = float(radius)
        except (TypeError, ValueError):
            raise ValueError("%s: radius must be a float or an (N,) tensor" % fn)
        if not (radius > 0.0 and math.isfinite(radius)):
            raise ValueError("%s: radius must be positive and finite, got %r" % (fn, radius))
    if lengths is not None:
        if not torch.is_tensor(lengths) or lengths.dim() != 1 or lengths.shape[0] != N or lengths.is_floating_point():
            raise ValueError("%s: lengths must be an integer tensor of shape (N,)" % fn)
        if any(l < 0 or l > P for l in host_lengths(lengths)):
            raise ValueError("%s: lengths must lie in [0, %d]" % (fn, P))
    if valid is not None and (not torch.is_tensor(valid) or tuple(valid.shape) != (N, P)):
        raise ValueError("%s: valid must be of shape (N, P)" % fn)
    if N * P >= _INDEX_LIMIT:
        raise ValueError("%s: %d clouds x %d points; the limit is 2^31 - 2 points in all" % (fn, N, P))
    for t in (points, valid, radius if torch.is_tensor(radius) else None):
        if t is not None and not t.is_cuda:
            raise _NotOnGpu("iso_points_amd: %s: tensors must be on the GPU; there is no CPU path" % fn)
    dev = points.device
    mask, sel, kept, _ = _eliminate(points.detach().float().contiguous(), frnn._as_lengths(lengths, N, P, dev),
                                    frnn._as_radius(radius, N, dev),
                                    None if valid is None else (valid != 0).to(torch.uint8).contiguous(), P)
    return mask.bool(), sel.long(), kept

