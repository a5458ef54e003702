"""Splat set-up and SurfaceSplatting.forward per Vrk mode (isotropic = default, invariant, anisotropic), median of 10
CUDA-event timed runs each, at the reference's working set (24 000 points, 1 view) and at 1 M points x 4 views (unit
sphere, 512 x 512, K = 8).  Per size: end-to-end forward() of every mode; per_point_info() of every mode on the filtered
packed clouds (neighbour search included); and the set-up kernels alone on given neighbours: iso_splat_setup,
iso_splat_vrk_h_global, iso_splat_setup_aniso (fused) and the unfused chain iso_pca_frames + iso_splat_setup_vrk.
Prints one JSON line (times in ms).  `--default-only`: forward() of the default mode alone (A/B against another commit).
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/vrk_bench.py`.
usage: python tools/vrk_bench.py [--default-only]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd import _lib  # noqa: E402
from iso_points_amd.levelset_sampling import with_host_lengths  # noqa: E402
from iso_points_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting  # noqa: E402
from oracle import splat_oracle as SO  # noqa: E402  (camera matrices only)

MODES = {"isotropic": dict(), "invariant": dict(Vrk_invariant=True), "anisotropic": dict(Vrk_isotropic=False)}
default_only = "--default-only" in sys.argv
dev = torch.device("cuda:0")
res = {"device": torch.cuda.get_device_name(0), "cases": []}
S, K = 512, 8
with torch.no_grad():
    for P, N in ((24000, 1), (1000000, 4)):
        g = torch.Generator().manual_seed(P)
        pts = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1).to(dev)
        nrm = pts.clone()
        views = torch.stack([SO.look_at_view(5.0, 20.0, 90.0 * i) for i in range(N)]).to(dev)
        projs = views @ SO.perspective(30.0).to(dev)
        c = {"points": P, "views": N}
        for mode, kw in MODES.items():
            if default_only and mode != "isotropic":
                continue
            ss = SurfaceSplatting(raster_settings=PointsRasterizationSettings(image_size=S, points_per_pixel=K, **kw))
            c["forward_%s_ms" % mode] = round(timeit(lambda: ss.forward(pts, nrm, cameras=(views, projs)), warm=3, rep=10), 4)
        if not default_only:
            ss = SurfaceSplatting(raster_settings=PointsRasterizationSettings(image_size=S, points_per_pixel=K))
            flags, off, lens = ss.filter_renderable(pts, nrm, views)
            tot, fl = sum(lens), [sum(lens[:i]) for i in range(N)]
            num = with_host_lengths(torch.tensor(lens, dtype=torch.int64, device=dev), lens)
            first = with_host_lengths(torch.tensor(fl, dtype=torch.int64, device=dev), fl)
            pf, nf = ss.compact(pts, flags, off, P, tot), ss.compact(nrm, flags, off, P, tot)
            c["rows"] = tot
            dbg = {}
            for mode, kw in MODES.items():
                ss.raster_settings = PointsRasterizationSettings(image_size=S, points_per_pixel=K, **kw)
                c["per_point_info_%s_ms" % mode] = round(timeit(lambda: ss.per_point_info(pf, nf, first, num, views, projs, debug=dbg),
                                                               warm=2, rep=10), 4)
            idx = dbg["knn_idx"]                                # (N, max rows, 8) of the anisotropic call above
            mx = idx.shape[1]
            padded = torch.zeros((N, mx, 3), dtype=torch.float32, device=dev)
            for v in range(N):
                padded[v, :lens[v]] = pf[fl[v]:fl[v] + lens[v]]
            from iso_points_amd import frnn
            from iso_points_amd.math_helper import pca_frames
            dists = frnn.frnn_grid_points(padded, padded, num, num, K=7, r=ss.frnn_radius)[0]
            outs = [torch.empty((tot, w), dtype=torch.float32, device=dev) for w in (3, 3, 1, 2, 1)]
            h = torch.full((tot,), 1e-3, dtype=torch.float32, device=dev)
            work = torch.empty((_lib.load().iso_splat_vrk_h_global_work_bytes(N),), dtype=torch.uint8, device=dev)
            p, st, o = _lib.ptr, _lib.stream(), [_lib.ptr(x) for x in outs]
            rows = torch.cat([torch.arange(lens[v], device=dev) + v * mx for v in range(N)])

            def unfused():
                curv, fr = pca_frames(padded, num, idx, False)
                _lib.call("iso_splat_setup_vrk", p(pf), p(fr.reshape(-1, 9)[rows].contiguous()), p(curv.reshape(-1, 3)[rows].contiguous()),
                          p(first), p(num), p(views), p(projs), N, mx, S, 1.0, 1.0, *o, st)

            def unfused_kernels_only():
                # one view: the padded layout IS the packed one, no gather in between
                curv, fr = pca_frames(padded, num, idx, False)
                _lib.call("iso_splat_setup_vrk", p(pf), p(fr), p(curv), p(first), p(num), p(views), p(projs), N, mx, S, 1.0, 1.0,
                          *o, st)

            c["kernel_setup_isotropic_ms"] = round(timeit(lambda: _lib.call(
                "iso_splat_setup", p(pf), p(nf), p(h), p(first), p(num), p(views), p(projs), N, mx, S, 1.0, 1.0, *o, st)), 4)
            c["kernel_h_global_ms"] = round(timeit(lambda: _lib.call(
                "iso_splat_vrk_h_global", p(dists), p(first), p(num), p(h), N, dists.shape[1], dists.shape[1], p(work), st)), 4)
            c["kernel_setup_aniso_fused_ms"] = round(timeit(lambda: _lib.call(
                "iso_splat_setup_aniso", p(pf), p(idx), mx, p(first), p(num), p(views), p(projs), N, S, 1.0, 1.0, *o, st)), 4)
            c["chain_pca_frames_plus_setup_vrk_ms"] = round(timeit(unfused_kernels_only if N == 1 else unfused), 4)
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
print(json.dumps(res))
