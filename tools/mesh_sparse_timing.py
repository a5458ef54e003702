"""Block-sparse mesh extraction (iso_points_amd.ops.sparse_level_set) against the dense path of the same build
(sdf_grid + marching_tetrahedra), on the SIREN 4 x 256 fitted to a sphere of radius 0.6 that tools/mesh_extract_timing.py
uses (DESIGN.md 3.4k records what this prints).

Dense at 512^3 and sparse at every size of --sizes, each the median [min, max] of `--rep` calls timed with device events
after 2 warm-up calls, in one process; at 512^3 the dense and the sparse calls alternate inside the timed loop, so both see
the same machine.  A call is what a user calls: allocations, host reads and torch's set operations on the block lists
included.  Per sparse size also, summed over the call's rounds and timed by device events inside the call:
  seed       the SDF at one test point per block (the band seeding)
  evaluate   the sample points of the new bricks and the fused value-only SIREN kernel
  count      iso_meshextract_sparse_count: table, classify, totals, scan
  emit       iso_meshextract_sparse_emit, its host read of the totals included
  other      call - the four: the block lists in torch and the host reads
and the counts: rounds, bricks cell-active and sampled, points evaluated, their share of the grid's points, workspace.
At 512^3 the sparse mesh sorted by its keys is compared with the dense mesh (`equals_dense`): faster and different is not
faster.  Writes one JSON document (times in ms) to --out and prints it.
usage: python tools/mesh_sparse_timing.py [--rep 10] [--sizes 512,1024,2048] [--fit 300] [--out profiles/mesh_sparse_timing.json]"""
import argparse
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iso_points_amd.ops import marching_tetrahedra, sdf_grid, sparse_level_set  # noqa: E402
from iso_points_amd.sdf_models import FusedSdf  # noqa: E402
from mesh_extract_timing import fitted  # noqa: E402

STAGES = ("seed", "evaluate", "count", "emit")


class StageClock:
    """sparse_level_set's _timer: device events around every stage of one call"""

    def __init__(self):
        self.spans = []

    @contextlib.contextmanager
    def __call__(self, name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.spans.append((name, a, b))

    def sums(self):
        torch.cuda.synchronize()
        out = dict.fromkeys(STAGES, 0.0)
        for name, a, b in self.spans:
            out[name] += a.elapsed_time(b)
        return out


def stats(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def grid_of(n):
    """sdf_grid's own axis, origin and spacing at n points per side"""
    import numpy as np
    axis64 = np.linspace(-0.5, 0.5, n) * 2.0
    return axis64.astype(np.float32), (float(axis64[0]),) * 3, (float(axis64[1] - axis64[0]),) * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rep", type=int, default=10)
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--fit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sparse_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_sparse_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    model, loss = fitted(dev, a.fit)
    sdf = FusedSdf(model, dev)
    res = {"device": torch.cuda.get_device_name(0), "rep": a.rep, "fit_steps": a.fit, "fit_l1": round(loss, 5), "dense": None,
           "sparse": []}

    def dense(n):
        values, org, spc = sdf_grid(sdf, n)
        return marching_tetrahedra(values, org, spc)

    def sparse(n, clock=None, keys=False):
        axis, org, spc = grid_of(n)
        ax = torch.from_numpy(axis).to(dev)
        return sparse_level_set(sdf, (n, n, n), org, spc, axes=[ax, ax, ax], return_info=True, return_keys=keys, _timer=clock)

    for n in (int(s) for s in a.sizes.split(",")):
        with_dense = n == 512
        for _ in range(2):
            sparse(n)
            if with_dense:
                dense(n)
        torch.cuda.synchronize()
        call, stage, dense_call, dense_grid, dense_mt = [], {k: [] for k in STAGES}, [], [], []
        for _ in range(a.rep):
            if with_dense:
                t_grid, (values, org, spc) = timed_once(lambda: sdf_grid(sdf, n))
                t_mt, _mesh = timed_once(lambda: marching_tetrahedra(values, org, spc))
                del values, _mesh
                dense_grid.append(t_grid)
                dense_mt.append(t_mt)
                dense_call.append(timed_once(lambda: dense(n))[0])
            clock = StageClock()
            t, out = timed_once(lambda: sparse(n, clock))
            call.append(t)
            for k, v in clock.sums().items():
                stage[k].append(v)
        info = out[-1]
        c = {"n": n, "grid_points": n ** 3, "verts": out[0].shape[0], "faces": out[1].shape[0], "call_ms": stats(call)}
        for k in STAGES:
            c[k + "_ms"] = stats(stage[k])
        c["other_ms"] = round(c["call_ms"][0] - sum(c[k + "_ms"][0] for k in STAGES), 4)
        c.update(info)
        c["evaluated_share"] = round(info["points_evaluated"] / n ** 3, 6)
        c["workspace_MB"] = round(info["workspace_bytes"] / 1e6, 1)
        del out
        if with_dense:
            v, f, vk, fc, _info = sparse(n, keys=True)
            dv, df = dense(n)
            order = torch.argsort(vk)
            new_index = torch.empty_like(order)
            new_index[order] = torch.arange(order.shape[0], device=dev)
            same = v.shape == dv.shape and f.shape == df.shape and torch.equal(v[order].view(torch.int32), dv.view(torch.int32)) \
                and torch.equal(new_index[f][torch.argsort(fc, stable=True)], df)
            c["equals_dense"] = bool(same)
            res["dense"] = {"n": n, "grid_points": n ** 3, "verts": dv.shape[0], "faces": df.shape[0],
                            "call_ms": stats(dense_call), "sdf_grid_ms": stats(dense_grid), "marching_tetrahedra_ms": stats(dense_mt)}
            c["dense_over_sparse"] = round(res["dense"]["call_ms"][0] / c["call_ms"][0], 2)
            c["dense_points_over_sparse_points"] = round(n ** 3 / info["points_evaluated"], 2)
            del v, f, vk, fc, dv, df
            print(res["dense"], file=sys.stderr, flush=True)
        res["sparse"].append(c)
        print(c, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
