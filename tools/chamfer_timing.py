"""Chamfer distance (iso_points_amd.loss.chamfer_distance) against the route that existed before it:
point_processing.knn_points(K = 1) both ways, a torch gather of the nearest points, torch reductions and torch autograd.
Cases: 100 k x 100 k and 1 M x 1 M points on two noisy unit spheres, forward alone and forward + backward.  The two
routes are timed in the same process, alternating, `rounds` times; every timing is the median of 10 device-event timed
calls after 2 warm-up calls, and the figure reported is the median over the rounds (the spread is printed with it).
Prints one JSON line (times in ms).
usage: python tools/chamfer_timing.py [--rounds 3] [--sizes 100000,1000000]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.loss import chamfer_distance  # noqa: E402
from iso_points_amd.point_processing import knn_points  # noqa: E402


def knn_route(x, y):
    """chamfer_distance(point_reduction = batch_reduction = "mean") from the K = 1 search and torch ops."""
    ix = knn_points(x, y, K=1).idx[..., 0]
    iy = knn_points(y, x, K=1).idx[..., 0]
    dx = (x - torch.gather(y, 1, ix.unsqueeze(-1).expand(-1, -1, 3))).square().sum(-1)
    dy = (y - torch.gather(x, 1, iy.unsqueeze(-1).expand(-1, -1, 3))).square().sum(-1)
    return (dx.mean(dim=1) + dy.mean(dim=1)).mean()


def fused_route(x, y):
    return chamfer_distance(x, y)[0]


def with_backward(route, x, y):
    x.grad = y.grad = None
    route(x, y).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/chamfer_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    for P in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator().manual_seed(P)
        clouds = []
        for _ in range(2):
            p = torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1)
            clouds.append((p + 0.01 * (torch.rand(1, P, 3, generator=g) - 0.5)).to(dev))
        x, y = clouds
        with torch.no_grad():
            v_new, v_old = fused_route(x, y).item(), knn_route(x, y).item()
        # faster and different is not faster: the two routes must agree at the size timed, values and gradients
        assert abs(v_new - v_old) <= 1e-5 * abs(v_old), (P, v_new, v_old)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        with_backward(fused_route, xg, yg)
        gx_new, gy_new = xg.grad.clone(), yg.grad.clone()
        with_backward(knn_route, xg, yg)
        for new, old in ((gx_new, xg.grad), (gy_new, yg.grad)):
            err = ((new - old).abs().max() / old.abs().max()).item()
            assert err <= 1e-5, (P, "gradients differ", err)
        t = {"fused_fwd": [], "knn_fwd": [], "fused_fwd_bwd": [], "knn_fwd_bwd": []}
        for _ in range(a.rounds):
            with torch.no_grad():
                t["fused_fwd"].append(timeit(lambda: fused_route(x, y)))
                t["knn_fwd"].append(timeit(lambda: knn_route(x, y)))
            t["fused_fwd_bwd"].append(timeit(lambda: with_backward(fused_route, xg, yg)))
            t["knn_fwd_bwd"].append(timeit(lambda: with_backward(knn_route, xg, yg)))
        c = {"points": P, "value_fused": v_new, "value_knn_route": v_old}
        for k, v in t.items():
            v = sorted(v)
            c[k + "_ms"] = round(v[len(v) // 2], 4)
            c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        c["speedup_fwd"] = round(c["knn_fwd_ms"] / c["fused_fwd_ms"], 3)
        c["speedup_fwd_bwd"] = round(c["knn_fwd_bwd_ms"] / c["fused_fwd_bwd_ms"], 3)
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
