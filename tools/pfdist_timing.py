"""Point-to-mesh face distance (iso_points_amd.loss.point_mesh_face_distance) against a chunked torch brute force of the
same closest-point formula on the same GPU: there is no earlier implementation to compare with.
Cases: the evaluation's own size (evaluation.py: 50 000 points sampled from a mesh, here against a ground-truth mesh of
80 k faces) and ten times that.  The mesh is a torus with a ripple, triangulated on a regular (u, v) grid; the points are
sampled on its faces and moved by 0.5 % of its size.
The brute force visits every (point, face) pair, so its time is linear in the number of queries: it is timed on `--sample`
queries of each direction against ALL targets and scaled to the full count (the JSON says so: "brute_scaled_ms"); the
tool first asserts that it agrees with the search on those queries.  Every timing of the search is the median of 10
device-event timed calls after 2 warm-up calls (the brute force: 3 after 1); the figure reported is the median over
`--rounds` alternating rounds, with the spread.
Prints one JSON line (times in ms).
usage: python tools/pfdist_timing.py [--rounds 3] [--scales 1,10] [--sample 2048]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.loss import face_point_distance, point_face_distance, point_mesh_face_distance  # noqa: E402

EVAL_POINTS, EVAL_FACES = 50000, 80000
PAIRS_PER_CHUNK = 1 << 22


def torus(n_faces, dev):
    """(verts (V,3), faces (F,3)) with F close to n_faces: nu x nv quads, nu = 2.5 nv."""
    nv = max(3, int(round(math.sqrt(n_faces / 5.0))))
    nu = max(3, int(round(2.5 * nv)))
    u = torch.arange(nu, device=dev, dtype=torch.float32) * (2 * math.pi / nu)
    v = torch.arange(nv, device=dev, dtype=torch.float32) * (2 * math.pi / nv)
    u, v = u[:, None].expand(nu, nv), v[None, :].expand(nu, nv)
    r = 0.4 + 0.05 * torch.sin(3 * u) * torch.cos(2 * v)
    verts = torch.stack([(1.0 + r * torch.cos(v)) * torch.cos(u), (1.0 + r * torch.cos(v)) * torch.sin(u),
                         r * torch.sin(v)], dim=-1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(nu, device=dev), torch.arange(nv, device=dev), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = torch.cat([torch.stack([a, b, c], dim=-1).reshape(-1, 3), torch.stack([a, c, d], dim=-1).reshape(-1, 3)])
    return verts, faces


def sample_points(tris, n, seed):
    g = torch.Generator(device=tris.device).manual_seed(seed)
    f = torch.randint(0, tris.shape[0], (n,), generator=g, device=tris.device)
    w = torch.rand(n, 2, generator=g, device=tris.device)
    s = w[:, :1].sqrt()
    b = torch.cat([1 - s, s * (1 - w[:, 1:]), s * w[:, 1:]], dim=1)
    noise = (torch.rand(n, 3, generator=g, device=tris.device) - 0.5) * 0.02
    return (tris[f] * b[:, :, None]).sum(dim=1) + noise


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_d2(p, tris):
    """The formula of include/isopoints.h section H (min_triangle_area = 0) for broadcast p (...,3), tris (...,3,3)."""
    v0, v1, v2 = tris[..., 0, :], tris[..., 1, :], tris[..., 2, :]

    def at(b0, b1, b2):
        r = p - ((b0[..., None] * v0 + b1[..., None] * v1) + b2[..., None] * v2)
        return dot3(r, r)

    def edge_t(a, b):
        d = b - a
        dd = dot3(d, d)
        t = (dot3(p - a, d) / dd).clamp(0.0, 1.0)
        return torch.where(dd > 0, t, torch.zeros_like(t))
    e1, e2 = v1 - v0, v2 - v0
    n = torch.cross(e1, e2, dim=-1)
    nn = dot3(n, n)
    w = p - v0
    b1 = dot3(torch.cross(w, e2.expand_as(w), dim=-1), n) / nn
    b2 = dot3(torch.cross(e1.expand_as(w), w, dim=-1), n) / nn
    b0 = (1.0 - b1) - b2
    inside = (nn > 0) & (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
    zero = torch.zeros_like(b0)
    t01, t12, t20 = edge_t(v0, v1), edge_t(v1, v2), edge_t(v2, v0)
    edges = torch.minimum(torch.minimum(at(1.0 - t01, t01, zero), at(zero, 1.0 - t12, t12)), at(t20, zero, 1.0 - t20))
    return torch.where(inside, at(b0, b1, b2), edges)


def brute_points(points, tris):
    """(P,) nearest-face distances, a chunk of points against all faces at a time."""
    step = max(1, PAIRS_PER_CHUNK // max(tris.shape[0], 1))
    return torch.cat([pair_d2(points[i:i + step, None, :], tris[None]).min(dim=1).values
                      for i in range(0, points.shape[0], step)])


def brute_faces(points, tris):
    step = max(1, PAIRS_PER_CHUNK // max(points.shape[0], 1))
    return torch.cat([pair_d2(points[:, None, :], tris[None, i:i + step]).min(dim=0).values
                      for i in range(0, tris.shape[0], step)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scales", default="1,10")
    ap.add_argument("--sample", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pfdist_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "sample": a.sample, "cases": []}
    for scale in (int(s) for s in a.scales.split(",")):
        verts, faces = torus(EVAL_FACES * scale, dev)
        tris = verts[faces].contiguous()
        P, T = EVAL_POINTS * scale, tris.shape[0]
        points = sample_points(tris, P, scale)
        first = torch.zeros(1, dtype=torch.int64, device=dev)
        first._iso_host, first._iso_host_version = [0], first._version
        ps, ts = min(a.sample, P), min(a.sample, T)
        sub_p = torch.randperm(P, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:ps]
        sub_t = torch.randperm(T, device=dev, generator=torch.Generator(device=dev).manual_seed(2))[:ts]
        with torch.no_grad():
            d_p = point_face_distance(points, first, tris, first, P)
            d_t = face_point_distance(points, first, tris, first, P)
            # faster and different is not faster: the search and the brute force must agree on the sampled queries
            for got, want in ((d_p[sub_p], brute_points(points[sub_p], tris)), (d_t[sub_t], brute_faces(points, tris[sub_t]))):
                err = (got - want).abs()
                assert bool((err <= 1e-5 * want + 1e-6).all()), (scale, err.max().item())
        mesh = (verts[None], faces[None])
        pg = points[None].clone().requires_grad_(True)

        def fwd_bwd():
            pg.grad = None
            point_mesh_face_distance(mesh, pg).backward()
        t = {"search_fwd": [], "brute_sample": [], "search_fwd_bwd": []}
        for _ in range(a.rounds):
            with torch.no_grad():
                t["search_fwd"].append(timeit(lambda: point_mesh_face_distance(mesh, points[None])))
                t["brute_sample"].append(timeit(lambda: (brute_points(points[sub_p], tris), brute_faces(points, tris[sub_t])),
                                                warm=1, rep=3))
            t["search_fwd_bwd"].append(timeit(fwd_bwd))
        c = {"points": P, "faces": T, "value": point_mesh_face_distance(mesh, points[None]).item()}
        for k, v in t.items():
            v = sorted(v)
            c[k + "_ms"] = round(v[len(v) // 2], 4)
            c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        # both directions visit P x T pairs; the sample visited ps x T + P x ts of them
        c["brute_scaled_ms"] = round(c["brute_sample_ms"] * (2.0 * P * T) / (float(ps) * T + float(P) * ts), 1)
        c["speedup_fwd"] = round(c["brute_scaled_ms"] / c["search_fwd_ms"], 1)
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
