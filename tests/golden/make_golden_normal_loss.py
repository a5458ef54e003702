"""Golden vectors for NormalLoss (DSS/training/losses.py:86-102): the reference's own estimate_pointcloud_normals
(make_golden_pca.load_mh: float64, batch_svd = torch.linalg.svd) is run AT GENERATION TIME on a noisy sphere of 1500 points
with perturbed normals, the three lines of NormalLoss.compute (:98-102) are evaluated on it and torch autograd gives the
gradients of the summed loss w.r.t. the points and the normals.  Only inputs and results are stored.

usage:  python tests/golden/make_golden_normal_loss.py        (writes tests/golden/normal_loss_K16.npz)
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

K = 16
P = 1500


def gen():
    from make_golden import npz
    from make_golden_pca import PC, load_mh
    MH = load_mh()
    g = torch.Generator().manual_seed(86102)
    sphere = F.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
    pts32 = (sphere + 0.05 * (torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5)).float()[None]
    nrm32 = (sphere + 0.3 * torch.randn(P, 3, generator=g, dtype=torch.float64)).float()[None]      # not unit length
    num = torch.tensor([P])
    pts = pts32.double().requires_grad_(True)
    nrm = nrm32.double().requires_grad_(True)
    _, _, knn = MH.estimate_pointcloud_local_coord_frames(PC(pts.detach(), num), neighborhood_size=K,
                                                          return_knn_result=True)
    # NormalLoss.compute, :98-102 (one cloud: padded_to_packed is the first row)
    normals_ref = MH.estimate_pointcloud_normals(PC(pts, num), neighborhood_size=K)
    loss = 1 - F.cosine_similarity(nrm[0], normals_ref[0]).abs()
    g_pts, g_nrm = torch.autograd.grad(loss.sum(), (pts, nrm))
    npz("normal_loss_K16.npz", points=pts32, normals=nrm32, idx=knn.idx.int(), K=K, loss=loss.detach(),
        grad_points=g_pts, grad_normals=g_nrm)


if __name__ == "__main__":
    gen()
