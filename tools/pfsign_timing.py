"""Sign of the point-to-mesh distance (iso_points_amd.loss.mesh_pseudonormals / point_mesh_sign) at the evaluation's own
size: 50 000 points against a ground-truth mesh of 80 k faces (the rippled torus of tools/pfdist_timing.py, the points
sampled on its faces and moved by 0.5 % of its size).  Timed next to each other: the forward face search alone
(nearest_faces), the pseudonormal build alone, the whole sign call with the build inside, and the sign call with the
vectors handed in (`normals=`: what a training loop with a fixed ground-truth mesh pays per step; the search is part of
it).  Before timing, the tool asserts that the signs agree with the generalised winding number on `--sample` points that
lie farther than 1e-4 from the mesh.
Every timing is the median of 10 device-event timed calls after 2 warm-up calls; the figure reported is the median over
`--rounds` alternating rounds, with the spread.  Prints one JSON line (times in ms).
usage: python tools/pfsign_timing.py [--rounds 3] [--sample 2048]"""
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
from pfdist_timing import EVAL_FACES, EVAL_POINTS, sample_points, torus  # noqa: E402
from iso_points_amd.loss import mesh_pseudonormals, nearest_faces, point_mesh_sign  # noqa: E402


def winding_number(points, tris):
    """Generalised winding number (Van Oosterom & Strackee), float64, a chunk of points against all faces at a time."""
    out = []
    step = max(1, (1 << 22) // max(tris.shape[0], 1))
    t = tris.double()
    for i in range(0, points.shape[0], step):
        q = points[i:i + step, None, :].double()
        a, b, c = t[None, :, 0] - q, t[None, :, 1] - q, t[None, :, 2] - q
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out.append(torch.atan2(num, den).sum(dim=1) / (2.0 * math.pi))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pfsign_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    verts, faces = torus(EVAL_FACES, dev)
    tris = verts[faces].contiguous()
    points = sample_points(tris, EVAL_POINTS, 1)
    mesh = (verts[None], faces[None])
    normals = mesh_pseudonormals(mesh)
    sign = point_mesh_sign(mesh, points, normals=normals)
    assert torch.equal(sign, point_mesh_sign(mesh, points))
    # fast and wrong is not fast: the winding number of the sampled points is the truth
    sub = torch.randperm(EVAL_POINTS, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:a.sample]
    w = winding_number(points[sub], tris)
    d2, _ = nearest_faces(points[sub], tris)
    far = d2.sqrt() > 1e-4
    # the torus of pfdist_timing.py is wound outward (its winding number is +1 inside): inside is -1
    want = torch.where(w > 0.5, -1.0, 1.0).float()
    wrong = int(((sign[sub] != want) & far).sum())
    assert wrong == 0, "%d of %d sampled signs disagree with the winding number" % (wrong, int(far.sum()))
    t = {"search_fwd": [], "normals_build": [], "sign_with_build": [], "sign_given_normals": []}
    with torch.no_grad():
        for _ in range(a.rounds):
            t["search_fwd"].append(timeit(lambda: nearest_faces(points, tris)))
            t["normals_build"].append(timeit(lambda: mesh_pseudonormals(mesh)))
            t["sign_with_build"].append(timeit(lambda: point_mesh_sign(mesh, points)))
            t["sign_given_normals"].append(timeit(lambda: point_mesh_sign(mesh, points, normals=normals)))
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "points": EVAL_POINTS, "faces": int(tris.shape[0]),
           "verts": int(verts.shape[0]), "inside_fraction": round(float((sign < 0).float().mean()), 4),
           "checked_against_winding_number": int(far.sum())}
    for k, v in t.items():
        v = sorted(v)
        res[k + "_ms"] = round(v[len(v) // 2], 4)
        res[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
