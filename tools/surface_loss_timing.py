"""The point regularisers (iso_points_amd.loss.surface_losses: ProjectionLoss + RepulsionLoss of DSS/training/losses.py) against
the same formulas composed from torch ops on the same GPU, the way the reference composes them: knn_others(return_nn=True),
frnn_gather for the neighbours' normals, about twenty element-wise ops and sums on (1,P,K) and (1,P,K,3) tensors.
One cloud (a jittered unit sphere with noisy normals), knn_k = 33, at 100 k and 1 M points.  The search is timed on its
own: both paths need it.  The sweeps (two mollifications and both losses) are timed without a gradient and with one
(forward + backward of the sum of both losses w.r.t. the points).  The tool first asserts that the two paths agree.
Every timing is the median of 10 device-event timed calls after 2 warm-up calls (the torch composition: 5 after 1); the
figure reported is the median over `--rounds` alternating rounds, with the spread.
Prints one JSON line (times in ms).
usage: python tools/surface_loss_timing.py [--rounds 3] [--sizes 100000,1000000]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.frnn import frnn_gather  # noqa: E402
from iso_points_amd.levelset_sampling import eps_denom  # noqa: E402
from iso_points_amd.loss import SurfaceKNN, surface_losses  # noqa: E402
from iso_points_amd.point_processing import knn_others  # noqa: E402

KNN_K, FILTER_SCALE, SIGMA = 33, 2.0, 0.75


def cloud(P, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, device=dev), dim=-1)
    pts = d * (1.0 + 0.02 * torch.randn(P, 1, generator=g, device=dev))
    return pts[None].contiguous(), (pts + 0.3 * torch.randn(P, 3, generator=g, device=dev))[None].contiguous()


def composed(points, normals, tree):
    """(projection (P,), repulsion (P,)) of one cloud from torch ops, as DSS/training/losses.py:300-515 composes them."""
    fs, inv_sigma2 = FILTER_SCALE, 1.0 / (SIGMA * SIGMA)
    unit = torch.nn.functional.normalize
    with torch.no_grad():
        d, x = tree.dists, tree.knn
        phi = (1 - d / (d[:, :, :1] * 2 * fs * fs)).clamp_min(0)
        phi = phi * phi
        phi = phi * phi

        def mollify(nrm, w):
            return (frnn_gather(nrm, tree.idx) * w[..., None]).sum(dim=-2) / eps_denom(w.sum(dim=-1, keepdim=True))
        n1 = mollify(normals, phi)
        diff = unit(frnn_gather(n1, tree.idx), dim=-1) - unit(n1, dim=-1)[:, :, None, :]
        nu = torch.exp(-(diff * diff).sum(dim=-1) * inv_sigma2)
        n2 = mollify(n1, phi * nu)
        ball = d > fs * d[:, :, :1] * 2.0
        w = (phi * nu).masked_fill(ball, 0.0)
        m = frnn_gather(n2, tree.idx)
    s = ((x - points.unsqueeze(-2)) * m).sum(dim=-1)
    den = eps_denom(w.sum(dim=-1))
    D = (w * s).sum(dim=-1) / den
    q = points + (s[..., None] * w[..., None] * m).sum(dim=-2) / den[..., None]
    with torch.no_grad():
        gap = x - q[:, :, None, :]
        sig = torch.exp(-(gap * gap).sum(dim=-1) * (points.shape[1] / 2.0))
        W = (nu * sig * (sig.sum(dim=-1, keepdim=True) + 1.0)).masked_fill(ball, 0.0)
    e = q[:, :, None, :] - x
    rep = -((e * e).sum(dim=-1) * W).sum(dim=-1) / eps_denom(W.sum(dim=-1))
    return (D * D)[0], rep[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/surface_loss_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "knn_k": KNN_K, "cases": []}
    for P in (int(s) for s in a.sizes.split(",")):
        points, normals = cloud(P, dev, P)
        found = knn_others(points, K=KNN_K - 1, return_nn=True)
        with_nn = SurfaceKNN(found.dists, found.idx, found.knn, points)
        gathered = SurfaceKNN(found.dists, found.idx, None, points)
        kw = dict(knn_k=KNN_K, filter_scale=FILTER_SCALE, sharpness_sigma=SIGMA)
        pg = points.clone().requires_grad_(True)

        def fused():
            return surface_losses(points, normals, knn=gathered, **kw)

        def fused_bwd():
            pg.grad = None
            r = surface_losses(pg, normals, knn=gathered, **kw)
            (r.projection.sum() + r.repulsion.sum()).backward()

        def torch_bwd():
            pg.grad = None
            pr, rp = composed(pg, normals, with_nn)
            (pr.sum() + rp.sum()).backward()
        # faster and different is not faster: values and gradients of the two paths must agree.  Both are float32 sums in
        # different orders, and a row whose weights all but vanish amplifies that: up to 0.1 % of the rows may differ
        def differing(got, want, rel, floor):
            bad = (got - want).abs() > rel * want.abs() + floor
            n_bad = int(bad.reshape(bad.shape[0], -1).any(dim=-1).sum()) if bad.dim() > 1 else int(bad.sum())
            assert n_bad <= P // 1000, (P, n_bad, (got - want).abs().max().item())
            return n_bad
        with torch.no_grad():
            f, (pr, rp) = fused(), composed(points, normals, with_nn)
        n_diff = differing(f.projection, pr, 1e-4, 1e-7) + differing(f.repulsion, rp, 1e-4, 1e-7)
        fused_bwd()
        g_fused = pg.grad.clone()
        torch_bwd()
        n_diff += differing(g_fused[0], pg.grad[0], 1e-3, 1e-5)
        t = {"search": [], "search_with_nn": [], "fused_fwd": [], "torch_fwd": [], "fused_fwd_bwd": [], "torch_fwd_bwd": []}
        for _ in range(a.rounds):
            with torch.no_grad():
                t["search"].append(timeit(lambda: knn_others(points, K=KNN_K - 1)))
                t["search_with_nn"].append(timeit(lambda: knn_others(points, K=KNN_K - 1, return_nn=True)))
                t["fused_fwd"].append(timeit(fused))
                t["torch_fwd"].append(timeit(lambda: composed(points, normals, with_nn), warm=1, rep=5))
            t["fused_fwd_bwd"].append(timeit(fused_bwd))
            t["torch_fwd_bwd"].append(timeit(torch_bwd, warm=1, rep=5))
        c = {"points": P, "projection_mean": f.projection.mean().item(), "repulsion_mean": f.repulsion.mean().item(),
             "rows_differing": n_diff}
        for k, v in t.items():
            v = sorted(v)
            c[k + "_ms"] = round(v[len(v) // 2], 4)
            c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        c["torch_over_fused_fwd"] = round(c["torch_fwd_ms"] / c["fused_fwd_ms"], 2)
        c["torch_over_fused_fwd_bwd"] = round(c["torch_fwd_bwd_ms"] / c["fused_fwd_bwd_ms"], 2)
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
        del found, with_nn, gathered
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
