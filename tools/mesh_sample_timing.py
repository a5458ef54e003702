"""Sampling points and normals on a mesh (iso_points_amd.ops.sample_points_from_meshes) against the torch formulation a user
would otherwise run on the same GPU: face areas -> torch.multinomial(S, replacement=True) -> two torch.rand -> the gathers
of the three vertices and the normal (what pytorch3d's own function does, without its packing).
Cases: the evaluation's own size (evaluation.py:50: 50 000 samples; here on a mesh of about 80 k faces) and 10^6 samples on
about 10^6 faces.  The mesh is the rippled torus of tools/pfdist_timing.py.  For each case the forward pass alone (points
and normals) and forward + backward to the vertices (the loss is the sum of points and normals times fixed weights).
Every timing is the median of 10 device-event timed calls after 2 warm-up calls; the figure reported is the median over
`--rounds` alternating rounds, with the spread.  The library timed is the one iso_points_amd._lib loads (ISO_DEV_LIB picks
a variant build).  Prints one JSON line (times in ms).
usage: python tools/mesh_sample_timing.py [--rounds 3]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from pfdist_timing import torus  # noqa: E402
from iso_points_amd import _lib  # noqa: E402
from iso_points_amd.ops import sample_points_from_meshes  # noqa: E402

CASES = ((50000, 80000), (1000000, 1000000))


def torch_sample(verts, faces, S):
    """(points (S,3), normals (S,3)) of one mesh, differentiable w.r.t. verts."""
    tris = verts[faces]
    m = torch.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0], dim=-1)
    length = m.norm(dim=-1)
    normals = m / length.clamp(min=2.220446e-16)[:, None]
    with torch.no_grad():
        f = torch.multinomial(0.5 * length, S, replacement=True)
        u, v = torch.rand(S, device=verts.device), torch.rand(S, device=verts.device)
        s = u.sqrt()
        w0, w1, w2 = 1.0 - s, s * (1.0 - v), s * v
    t = tris[f]
    return w0[:, None] * t[:, 0] + w1[:, None] * t[:, 1] + w2[:, None] * t[:, 2], normals[f]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_sample_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "lib": os.path.relpath(_lib.LIB_PATH, ROOT),
           "cases": []}
    for S, n_faces in CASES:
        verts, faces = torus(n_faces, dev)
        g = torch.Generator(device=dev).manual_seed(S)
        Wp, Wn = torch.randn(S, 3, generator=g, device=dev), torch.randn(S, 3, generator=g, device=dev)
        vg = verts.clone().requires_grad_(True)
        mesh, mesh_g = (verts[None], faces[None]), (vg[None], faces[None])

        def fused_fwd_bwd():
            vg.grad = None
            p, n = sample_points_from_meshes(mesh_g, S, return_normals=True)
            ((p[0] * Wp).sum() + (n[0] * Wn).sum()).backward()

        def torch_fwd_bwd():
            vg.grad = None
            p, n = torch_sample(vg, faces, S)
            ((p * Wp).sum() + (n * Wn).sum()).backward()
        # both are samplers of the same distribution: the mean point of the surface must agree to sampling noise
        with torch.no_grad():
            mean_f = sample_points_from_meshes(mesh, S)[0].mean(dim=0)
            mean_t = torch_sample(verts, faces, S)[0].mean(dim=0)
            assert (mean_f - mean_t).abs().max().item() < 6.0 * 1.5 / S ** 0.5, (mean_f, mean_t)
        t = {"fused_fwd": [], "torch_fwd": [], "fused_fwd_bwd": [], "torch_fwd_bwd": []}
        for _ in range(a.rounds):
            with torch.no_grad():
                t["fused_fwd"].append(timeit(lambda: sample_points_from_meshes(mesh, S, return_normals=True)))
                t["torch_fwd"].append(timeit(lambda: torch_sample(verts, faces, S)))
            t["fused_fwd_bwd"].append(timeit(fused_fwd_bwd))
            t["torch_fwd_bwd"].append(timeit(torch_fwd_bwd))
        c = {"samples": S, "faces": int(faces.shape[0])}
        for k, v in t.items():
            v = sorted(v)
            c[k + "_ms"] = round(v[len(v) // 2], 4)
            c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        c["speedup_fwd"] = round(c["torch_fwd_ms"] / c["fused_fwd_ms"], 2)
        c["speedup_fwd_bwd"] = round(c["torch_fwd_bwd_ms"] / c["fused_fwd_bwd_ms"], 2)
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
