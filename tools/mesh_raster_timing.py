"""Mesh rasterisation (iso_points_amd.mesh_raster) pass by pass, and against the same rule written in chunked torch on the
same GPU: the reference's own rasteriser (pytorch3d, CUDA only) cannot run here, so this is the only comparison there is.
Cases: icosphere(6) (81 920 faces) and icosphere(7) (327 680) seen by look_at_view(2.7, 20, 30) / perspective(60), at
512 x 512 with K = 5 (scripts/create_mvr_data_from_mesh.py) and at 256 x 256 with K = 4 (SignedDistanceLoss's layers).
Per pass (count + tile offsets, the host read of the pair total, fill, raster) the median of `--rep` calls timed with
device events after 2 warm-up calls, in one process; `total_ms` is the whole call from the first event to the last.
The torch brute force visits every (pixel, face) pair, so its time is linear in the number of faces: it is timed on the
first `--sample` front faces against ALL pixels and scaled to the mesh ("brute_scaled_ms"); the tool first asserts that it
agrees with the kernels on those faces.  `heaviest_tile` is the longest face list of a tile and `mean_tile` the mean over
the tiles that have one: the raster pass lasts as long as its heaviest workgroup.
Prints one JSON line (times in ms).
usage: python tools/mesh_raster_timing.py [--rep 10] [--levels 6,7] [--sample 2048]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd import _lib, cameras  # noqa: E402
from iso_points_amd.mesh_raster import MeshRasterizer, _raster_packed  # noqa: E402

PAIRS_PER_CHUNK = 1 << 24
SETTINGS = ((512, 5), (256, 4))


def icosphere(level):
    """(verts (V,3) f32, faces (F,3) int64) of the unit icosphere, outward wound: 20 * 4^level faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(3, -1) + len(v)                       # midpoints of (a,b), (b,c), (c,a)
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([b, m[1], m[0]], 1), np.stack([c, m[2], m[1]], 1),
                            np.stack([m[0], m[1], m[2]], 1)])
        v = np.concatenate([v, mid])
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f)


def brute(tris, S, K):
    """The rule of include/isopoints.h section M (perspective_correct off) in torch, a chunk of faces against all pixels at a
    time -> (pix_to_face (S,S,K) int64, zbuf (S,S,K))."""
    dev = tris.device
    cen = 1.0 - (2 * torch.arange(S, device=dev, dtype=torch.float32) + 1) / S
    py, px = [g.reshape(-1, 1) for g in torch.meshgrid(cen, cen, indexing="ij")]
    best_z = torch.full((S * S, K), float("inf"), device=dev)
    best_i = torch.full((S * S, K), -1, dtype=torch.int64, device=dev)
    step = max(1, PAIRS_PER_CHUNK // (S * S))
    for i in range(0, tris.shape[0], step):
        t = tris[i:i + step]
        x0, y0, z0, x1, y1, z1, x2, y2, z2 = [t[:, a, b][None] for a in range(3) for b in range(3)]
        area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
        skip = ~torch.isfinite(t.reshape(-1, 9)).all(dim=1)[None] | ~(area.abs() > 1e-8) | (torch.maximum(torch.maximum(z0, z1), z2) < 0)
        w0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) / area
        w1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) / area
        w2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) / area
        pz = (w0 * z0 + w1 * z1) + w2 * z2
        ok = (w0 > 0) & (w1 > 0) & (w2 > 0) & ~skip & (pz >= 0) & torch.isfinite(pz)
        z = torch.cat([best_z, torch.where(ok, pz, torch.full_like(pz, float("inf")))], dim=1)
        ids = torch.cat([best_i, torch.arange(i, i + t.shape[0], device=dev).expand(S * S, -1)], dim=1)
        best_z, sel = torch.topk(z, K, dim=1, largest=False, sorted=True)
        best_i = torch.gather(ids, 1, sel)
    hit = torch.isfinite(best_z)
    return torch.where(hit, best_i, torch.full_like(best_i, -1)).reshape(S, S, K), \
        torch.where(hit, best_z, torch.full_like(best_z, -1.0)).reshape(S, S, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rep", type=int, default=10)
    ap.add_argument("--levels", default="6,7")
    ap.add_argument("--sample", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_raster_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    view = cameras.look_at_view(2.7, 20.0, 30.0)[None].to(dev)
    cams = (view, view @ cameras.perspective(60.0).to(dev))
    res = {"device": torch.cuda.get_device_name(0), "rep": a.rep, "sample": a.sample, "cases": []}
    passes = ("count", "read", "fill", "raster")
    for level in (int(s) for s in a.levels.split(",")):
        v, f = icosphere(level)
        ndc, first, num, _ = MeshRasterizer(cams).transform((v[None].to(dev), f[None].to(dev)))
        F = ndc.shape[0]
        area = (ndc[:, 2, 0] - ndc[:, 0, 0]) * (ndc[:, 1, 1] - ndc[:, 0, 1]) - (ndc[:, 2, 1] - ndc[:, 0, 1]) * (ndc[:, 1, 0] - ndc[:, 0, 0])
        front = ndc[area > 0][:a.sample].contiguous()
        one = torch.tensor([front.shape[0]], dtype=torch.int64, device=dev)
        for S, K in SETTINGS:
            # faster and different is not faster: kernels and brute force must agree on the sampled faces
            fr = _raster_packed(front, torch.zeros_like(one), one, S, K, False, False)
            bi, bz = brute(front, S, K)
            same = (fr.pix_to_face[0] == bi).all(dim=-1)
            assert same.float().mean().item() > 0.999, (level, S, same.float().mean().item())
            assert torch.equal(fr.zbuf[0][same], bz[same])
            ts = {p: [] for p in passes + ("total",)}
            pairs = 0
            for r in range(a.rep + 2):
                ev = {}
                _raster_packed(ndc, first, num, S, K, False, False, timings=ev)
                torch.cuda.synchronize()
                pairs = ev.pop("pairs")
                if r >= 2:
                    prev = "begin"
                    for p in passes:
                        ts[p].append(ev[prev].elapsed_time(ev[p]))
                        prev = p
                    ts["total"].append(ev["begin"].elapsed_time(ev["raster"]))
            lib, p = _lib.load(), _lib.ptr
            T = lib.iso_splat_tiles_per_side(S)
            cnt = torch.zeros((T * T + 1,), dtype=torch.int32, device=dev)
            _lib.call("iso_meshraster_count", p(ndc), p(first), p(num), 1, F, S, 0, p(cnt), _lib.stream())
            c = {"level": level, "faces": F, "image_size": S, "faces_per_pixel": K, "pairs": pairs,
                 "heaviest_tile": int(cnt.max().item()), "mean_tile": round(cnt[cnt > 0].float().mean().item(), 1),
                 "covered": round((_raster_packed(ndc, first, num, S, K, False, False).pix_to_face[..., 0] >= 0).float().mean().item(), 4)}
            for k, vals in ts.items():
                vals = sorted(vals)
                c[k + "_ms"] = round(vals[len(vals) // 2], 4)
                c[k + "_min_max_ms"] = [round(vals[0], 4), round(vals[-1], 4)]
            c["brute_sample_ms"] = round(timeit(lambda: brute(front, S, K), warm=1, rep=3), 3)
            c["brute_scaled_ms"] = round(c["brute_sample_ms"] * F / front.shape[0], 1)
            c["speedup"] = round(c["brute_scaled_ms"] / c["total_ms"], 1)
            res["cases"].append(c)
            print(c, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
