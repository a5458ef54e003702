"""Golden vectors for the local-frame estimator (DSS/utils/mathHelper.py:43-119): the reference's own
estimate_pointcloud_local_coord_frames is imported from the checkout AT GENERATION TIME and run in float64 on
float32-rounded inputs; only inputs and results are stored (pca_*.npz).  Its third-party pieces are absent here and are
set as module globals: knn_points = the oracle's brute force (same (d2, index) order as this package's exact kNN),
batch_svd = float64 torch.linalg.svd returning (U, S, V) with V = Vh^T, and _disambiguate_vector_directions = pytorch3d's
four-line rule.  The remove_outliers mask (point_processing.py:23-26) is stored at tolerance 0.05 for K = 16 and K = 31.

usage:  python tests/golden/make_golden_pca.py        (writes tests/golden/pca_*.npz)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, HERE)

TOLERANCE = 0.05


def _disambiguate_vector_directions(pcl, knns, vecs):
    df = knns - pcl[:, :, None]
    proj = (vecs[:, :, None] * df).sum(3)
    n_pos = (proj > 0).type_as(knns).sum(2, keepdim=True)
    flip = (n_pos < (0.5 * knns.shape[2])).type_as(knns)
    return (1.0 - 2.0 * flip) * vecs


def batch_svd(x):
    U, S, Vh = torch.linalg.svd(x, full_matrices=False)
    return U, S, Vh.transpose(-1, -2)


class PC(object):
    def __init__(self, pts, num):
        self._p, self._n = pts, num

    def points_padded(self):
        return self._p

    def num_points_per_cloud(self):
        return self._n


def load_mh():
    from make_golden import install_shims
    install_shims()
    sys.path.insert(0, REF)
    import importlib
    from oracle import iso_oracle as O
    MH = importlib.import_module("DSS.utils.mathHelper")

    def convert_pointclouds_to_tensor(p):
        if torch.is_tensor(p):
            return p, torch.full((p.shape[0],), p.shape[1], dtype=torch.long)
        return p.points_padded(), p.num_points_per_cloud()

    def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, return_nn=True):
        r = O.knn_points(p1.float(), p2.float(), lengths1, lengths2, K=K, return_nn=False)
        knn = torch.stack([p2[b][r.idx[b]] for b in range(p2.shape[0])]) if return_nn else None
        return O.KNN(dists=r.dists, idx=r.idx, knn=knn)

    MH.knn_points = knn_points
    MH.batch_svd = batch_svd
    MH.convert_pointclouds_to_tensor = convert_pointclouds_to_tensor
    MH._disambiguate_vector_directions = _disambiguate_vector_directions
    return MH


def cases():
    g = torch.Generator().manual_seed(2024)

    def sphere(P, jitter):
        p = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
        return p + jitter * (torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5)

    def cube(P, jitter):
        # points on the surface of [-1, 1]^3 (faces, edges and corners), uniformly over the six faces
        u = torch.rand(P, 3, generator=g, dtype=torch.float64) * 2 - 1
        face = torch.randint(0, 6, (P,), generator=g)
        ax, sgn = face % 3, (face // 3).double() * 2 - 1
        u[torch.arange(P), ax] = sgn
        return u + jitter * (torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5)

    def scatter(x, n):
        # n stray points inside the cloud's box replace its last rows: what remove_outliers is meant to find
        lo, hi = x.amin(dim=0), x.amax(dim=0)
        x[-n:] = lo + (hi - lo) * torch.rand(n, 3, generator=g, dtype=torch.float64)
        return x

    one = lambda x: (x.float()[None], torch.tensor([x.shape[0]]))   # noqa: E731
    out = [("sphere_K8", one(scatter(sphere(1500, 0.05), 40)), 8),
           ("sphere_K16", one(scatter(sphere(1500, 0.05), 40)), 16),
           ("cube_K12", one(scatter(cube(1500, 0.01), 40)), 12)]
    a, b = scatter(sphere(1200, 0.05), 30), scatter(0.5 * cube(700, 0.02) + 0.3, 20)
    pts = torch.zeros(2, 1200, 3)
    pts[0], pts[1, :700] = a.float(), b.float()
    out.append(("ragged_K16", (pts, torch.tensor([1200, 700])), 16))
    out.append(("translated_K16", one(scatter(0.6 * sphere(1500, 0.05) + torch.tensor([20.0, -7.0, 5.0], dtype=torch.float64),
                                                    40)), 16))
    return out


def gen_pca():
    from make_golden import npz
    MH = load_mh()
    for name, (pts32, num), K in cases():
        pts = pts32.double()
        arrays = {"points": pts32, "num_points": num, "K": K, "tolerance": TOLERANCE}
        for dis in (True, False):
            curv, frames, knn = MH.estimate_pointcloud_local_coord_frames(PC(pts, num), neighborhood_size=K,
                                                                          disambiguate_directions=dis, return_knn_result=True)
            tag = "dis" if dis else "raw"
            arrays["curvature_" + tag] = curv
            arrays["frames_" + tag] = frames
            arrays["idx"] = knn.idx.int()          # int32 on disk: the indices are < 2^31
        inside = torch.arange(pts.shape[1])[None, :] < num[:, None]
        for k_out in (16, 31):
            variance, _ = MH.estimate_pointcloud_local_coord_frames(PC(pts, num), neighborhood_size=k_out)
            ratio = variance[..., 0] / torch.sum(variance, dim=-1)                       # point_processing.py:25
            arrays["outlier_ratio_K%d" % k_out] = ratio
            arrays["outlier_mask_K%d" % k_out] = (ratio < TOLERANCE) & inside
        npz("pca_%s.npz" % name, **arrays)


if __name__ == "__main__":
    gen_pca()
