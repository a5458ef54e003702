"""Local frames (math_helper.estimate_pointcloud_local_coord_frames): the exact kNN query alone, kNN + frames (the whole
estimator) and the frames kernel alone (iso_pca_frames on a given index, with and without the sign rule), median of 10
CUDA-event timed runs each.  Cases: the trainer's call (5 000 FPS points, K = 12), the reference's iso-point working set
(24 000 points, K = 8 / 16) and 1 M points (K = 16 / 32), noisy unit spheres.  Prints one JSON line (times in ms).
usage: python tools/pca_bench.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames, pca_frames  # noqa: E402
from iso_points_amd.point_processing import knn_points  # noqa: E402

dev = torch.device("cuda:0")
res = {"device": torch.cuda.get_device_name(0), "cases": []}
with torch.no_grad():
    for P, K in ((5000, 12), (24000, 8), (24000, 16), (1000000, 16), (1000000, 32)):
        g = torch.Generator().manual_seed(P + K)
        p = torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1)
        x = (p + 0.01 * (torch.rand(1, P, 3, generator=g) - 0.5)).to(dev)
        num = torch.tensor([P], device=dev)
        idx = knn_points(x, x, num, num, K=K).idx
        t_knn = timeit(lambda: knn_points(x, x, num, num, K=K), warm=2, rep=10)
        t_all = timeit(lambda: estimate_pointcloud_local_coord_frames(x, neighborhood_size=K), warm=2, rep=10)
        t_fr = timeit(lambda: pca_frames(x, num, idx, True), warm=2, rep=10)
        t_raw = timeit(lambda: pca_frames(x, num, idx, False), warm=2, rep=10)
        c = {"points": P, "K": K, "knn_ms": round(t_knn, 4), "knn_plus_frames_ms": round(t_all, 4),
             "frames_ms": round(t_fr, 4), "frames_no_sign_rule_ms": round(t_raw, 4),
             "frames_ns_per_point": round(t_fr * 1e6 / P, 3)}
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
print(json.dumps(res))
