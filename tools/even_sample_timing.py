"""Even sampling of a mesh (iso_points_amd.ops.sample_points_from_meshes_even) stage by stage: the draw of 3 S samples, the
grid build on them, the elimination rounds (with their host reads) and the compaction, plus the whole call.
Cases: S = 10 000 of 30 000 draws on the icosphere of level 5 (20 480 faces), the reference's working set
(config.py:224-232), and S = 1 000 000 of 3 000 000 on the same mesh.  The radius is the default sqrt(area / (3 S)).
Per case it also reports the rounds the elimination needed, the host reads, the points kept, and the time of every single
round (one launch per call, the number left read after each: what compacting the undecided list between batches could save
is the sum of the later rounds).  At the small size it runs the host path the operator replaces on the same points --
scipy's cKDTree.query_pairs plus the serial loop over the pairs, as trimesh / the reference's data pipeline do it on the CPU --
once, timed by the wall clock, copies included: for orientation only, it is another machine part and another rule.
Every device timing is the median of 10 device-event timed calls after 2 warm-up calls; the figure reported is the median
over `--rounds` rounds, with the spread.  Prints one JSON line (times in ms).
usage: python tools/even_sample_timing.py [--rounds 3] [--no-large]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools_common import timeit  # noqa: E402
from mesh_sample_oracle import icosphere  # noqa: E402
from iso_points_amd import _lib, frnn, point_processing  # noqa: E402
from iso_points_amd.ops import sample_points_from_meshes, sample_points_from_meshes_even  # noqa: E402

CASES = (10000, 1000000)


def host_path(points, r):
    """cKDTree pair query + the serial rule on the host: (seconds, number kept)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = points.cpu().numpy().astype(np.float64)
    pairs = cKDTree(p).query_pairs(float(r), output_type="ndarray")
    lower = [[] for _ in range(len(p))]
    for i, j in pairs:                                  # i < j
        lower[j].append(i)
    kept = np.zeros(len(p), dtype=bool)
    for s in range(len(p)):
        kept[s] = not any(kept[j] for j in lower[s])
    return time.perf_counter() - t0, int(kept.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/even_sample_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v, f = icosphere(5)
    mesh = (torch.from_numpy(v.astype(np.float32))[None].to(dev), torch.from_numpy(f)[None].to(dev))
    area = float(0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum())
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "lib": os.path.relpath(_lib.LIB_PATH, ROOT),
           "faces": int(len(f)), "rounds_per_batch": point_processing.ROUNDS_PER_BATCH, "cases": []}
    lib, p = _lib.load(), _lib.ptr
    for S in CASES[:1] if a.no_large else CASES:
        D = 3 * S
        r = float(np.float32(np.sqrt(area / (3.0 * S))))
        gen = lambda: torch.Generator().manual_seed(S)  # noqa: E731
        pts, face, _ = sample_points_from_meshes(mesh, D, return_faces=True, generator=gen())
        pts = pts.contiguous()
        lens = torch.full((1,), D, dtype=torch.int64, device=dev)
        rad = torch.full((1,), r, dtype=torch.float32, device=dev)
        valid = (face >= 0).to(torch.uint8).contiguous()
        grid = frnn.build_grid(pts, lens, rad)
        ws_bytes = lib.iso_disk_workspace_bytes(1, D)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        left = torch.empty((1,), dtype=torch.int32, device=dev)
        mask = torch.empty((1, D), dtype=torch.uint8, device=dev)
        sel = torch.empty((1, S), dtype=torch.int32, device=dev)
        kept = torch.empty((1,), dtype=torch.int64, device=dev)
        reads = [0]

        def begin():
            _lib.call("iso_disk_begin", p(grid.sorted_points), p(grid.sorted_idx), p(lens), p(valid), 1, D, p(ws), ws_bytes,
                      _lib.stream())

        def some_rounds(first, n):
            _lib.call("iso_disk_rounds", p(lens), p(grid.off), p(grid.params), p(rad), 1, D, grid.g_stride, first, n, p(left),
                      p(ws), ws_bytes, _lib.stream())

        def eliminate():
            begin()
            done, reads[0] = 0, 0
            while True:
                some_rounds(done, point_processing.ROUNDS_PER_BATCH)
                done += point_processing.ROUNDS_PER_BATCH
                reads[0] += 1
                if int(left.item()) == 0:
                    return

        def select():
            _lib.call("iso_disk_select", 1, D, S, p(mask), p(sel), p(kept), p(ws), ws_bytes, _lib.stream())

        # the rounds one by one: time and what each leaves open
        begin()
        per_round, open_after = [], []
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            some_rounds(len(per_round), 1)
            e1.record()
            torch.cuda.synchronize()
            per_round.append(round(e0.elapsed_time(e1), 4))
            open_after.append(int(left.item()))
            if open_after[-1] == 0:
                break
        select()
        n_kept_all = int(mask.sum())
        t = {"draw": [], "grid": [], "rounds": [], "select": [], "whole_call": []}
        with torch.no_grad():
            for _ in range(a.rounds):
                t["draw"].append(timeit(lambda: sample_points_from_meshes(mesh, D, return_faces=True, generator=gen())))
                t["grid"].append(timeit(lambda: frnn.build_grid(pts, lens, rad)))
                t["rounds"].append(timeit(eliminate))
                t["select"].append(timeit(select))
                t["whole_call"].append(timeit(lambda: sample_points_from_meshes_even(mesh, S, generator=gen())))
        out, num = sample_points_from_meshes_even(mesh, S, generator=gen())
        assert int(num[0]) == min(S, n_kept_all) and torch.equal(out[0, :int(num[0])], pts[0][sel[0, :int(num[0])].long()])
        c = {"S": S, "draws": D, "radius": r, "kept_of_draws": n_kept_all, "num_points": int(num[0]),
             "rounds_needed": len(per_round), "host_reads_per_call": reads[0], "per_round_ms": per_round,
             "open_after_round": open_after}
        for k, vals in t.items():
            vals = sorted(vals)
            c[k + "_ms"] = round(vals[len(vals) // 2], 4)
            c[k + "_min_max_ms"] = [round(vals[0], 4), round(vals[-1], 4)]
        if S == CASES[0]:
            try:
                sec, n_host = host_path(pts[0], r)
                c["host_ckdtree_serial_ms"] = round(sec * 1e3, 1)
                c["host_kept"] = n_host         # float64 distances, d < r or <= r as scipy has it: may differ by a few
            except ImportError:
                c["host_ckdtree_serial_ms"] = None
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
