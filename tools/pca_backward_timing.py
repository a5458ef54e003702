"""NormalLoss (iso_points_amd.loss.NormalLoss, DSS/training/losses.py:86-102), forward + backward w.r.t. the points and the
normals, against the same loss written in torch on the same GPU: the (P,K,3) gather of the neighbours, the centred
covariances, torch.linalg.eigh and autograd through all of it.  One cloud (a jittered unit sphere with noisy normals),
K = 16, at 24 000 and 1 M points.  Both paths run the same exact kNN search inside the timed call, and the search is timed
on its own beside them.  The tool first asserts that the two paths agree on the values and on the point gradients.
Every timing is the median of 10 device-event timed calls after 2 warm-up calls (the torch composition: 3 after 1); the
figure reported is the median over `--rounds` alternating rounds, with the spread.
Prints one JSON line per size (times in ms).
usage: python tools/pca_backward_timing.py [--rounds 3] [--sizes 24000,1000000]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.loss import NormalLoss  # noqa: E402
from iso_points_amd.point_processing import knn_points  # noqa: E402

K = 16


def cloud(P, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, device=dev), dim=-1)
    pts = d * (1.0 + 0.02 * torch.randn(P, 1, generator=g, device=dev))
    return pts[None].contiguous(), (d + 0.3 * torch.randn(P, 3, generator=g, device=dev))[None].contiguous()


def composed(points, normals):
    """The per-point loss of one cloud from torch ops: kNN, gather, covariance, eigh, cosine."""
    idx = knn_points(points, points, K=K).idx[0]
    X = points[0][idx]                                                   # (P,K,3)
    D = X - X.mean(dim=1, keepdim=True)
    C = torch.einsum("pki,pkj->pij", D, D) / K
    _, V = torch.linalg.eigh(C)
    return 1 - torch.nn.functional.cosine_similarity(normals[0], V[:, :, 0]).abs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="24000,1000000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pca_backward_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    loss = NormalLoss(reduction="sum", neighborhood_size=K)
    for P in (int(s) for s in a.sizes.split(",")):
        points, normals = cloud(P, dev, P)
        pg, ng = points.clone().requires_grad_(True), normals.clone().requires_grad_(True)

        def fused_bwd():
            pg.grad, ng.grad = None, None
            loss((pg, ng)).backward()

        def torch_bwd():
            pg.grad, ng.grad = None, None
            composed(pg, ng).sum().backward()
        # faster and different is not faster: values and point gradients must agree, up to 0.1 % of the rows (two float32
        # eigensolvers; rows whose two smallest eigenvalues nearly meet amplify the difference)
        with torch.no_grad():
            v_f, v_t = NormalLoss(reduction="none", neighborhood_size=K)((points, normals)), composed(points, normals)
        n_diff = int(((v_f - v_t).abs() > 1e-4).sum())
        fused_bwd()
        g_f = pg.grad.clone()
        torch_bwd()
        g_t = pg.grad.clone()
        # the gradients by the median over the points: where the two smallest eigenvalues nearly meet (the radial noise is
        # of the size of the neighbourhoods here) the gradient is ill-conditioned and two float32 eigensolvers differ freely;
        # the share of such points is reported, not judged -- tests/test_pca_backward_gpu.py judges the kernel against float64
        per_point = (g_f - g_t)[0].norm(dim=-1) / g_t[0].norm(dim=-1).clamp_min(1e-30)
        g_rel = float(per_point.median())
        g_tail = float((per_point > 1e-2).float().mean())
        assert n_diff <= max(P // 1000, 2) and g_rel <= 1e-3, (P, n_diff, g_rel, g_tail)
        t = {"search": [], "fused_fwd_bwd": [], "torch_fwd_bwd": []}
        for _ in range(a.rounds):
            with torch.no_grad():
                t["search"].append(timeit(lambda: knn_points(points, points, K=K)))
            t["fused_fwd_bwd"].append(timeit(fused_bwd))
            t["torch_fwd_bwd"].append(timeit(torch_bwd, warm=1, rep=3))
        c = {"device": torch.cuda.get_device_name(0), "points": P, "K": K, "rounds": a.rounds,
             "loss_mean": float(v_f.mean()), "rows_differing": n_diff,
             "grad_median_rel_diff_between_paths": g_rel, "grad_share_beyond_1e-2": g_tail}
        for k, v in t.items():
            v = sorted(v)
            c[k + "_ms"] = round(v[len(v) // 2], 4)
            c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        c["torch_over_fused"] = round(c["torch_fwd_bwd_ms"] / c["fused_fwd_bwd_ms"], 2)
        print(json.dumps(c), flush=True)
        del pg, ng, g_f, g_t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
