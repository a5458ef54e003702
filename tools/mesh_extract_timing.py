"""Mesh extraction (iso_points_amd.ops.sdf_grid + marching_tetrahedra) stage by stage on a SIREN 4 x 256 fitted to a
sphere of radius 0.6, at 128^3 and 512^3 (DESIGN.md 3.4j records what this prints).  The parent of the commit that added
the extraction has nothing to compare with, so the figures stand alone.

Per size the median [min, max] of `--rep` calls timed with device events after 2 warm-up calls, in one process:
  sdf_grid   the grid points and the fused value-only SIREN kernel
  count      iso_meshextract_count: classify + totals + scan
  scan       iso_prefix_sum alone on arrays of the same size (2 rows of nx ny nz counters)
  classify   count - scan (medians): pass 1 with its 64-bit totals
  emit       iso_meshextract_emit, its 16-byte read of the totals included
  call       marching_tetrahedra as a user calls it: allocations, both host reads, the int64 copy of the faces
`classify_volume_GBps` is the volume's size (4 bytes per point) over the classify time -- the effective rate against what
the pass has to read; `classify_traffic_GBps` counts what it moves (4 read + 9 written per point).
Prints one JSON line (times in ms).
usage: python tools/mesh_extract_timing.py [--rep 10] [--sizes 128,512] [--fit 300]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iso_points_amd import _lib  # noqa: E402
from iso_points_amd.ops import marching_tetrahedra, sdf_grid  # noqa: E402
from iso_points_amd.sdf_models import FusedSdf, Siren  # noqa: E402


def fitted(dev, steps):
    torch.manual_seed(0)
    model = Siren(hidden_size=256, n_layers=3).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    for _ in range(steps):
        x = torch.rand(8192, 3, device=dev) * 2 - 1
        loss = (model(x).sdf[:, 0] - (x.norm(dim=1) - 0.6)).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return model, loss.item()


def timed(fn, rep):
    """median, min, max of `rep` device-event timings after 2 warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rep", type=int, default=10)
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--fit", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_extract_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    model, loss = fitted(dev, a.fit)
    sdf = FusedSdf(model, dev)
    lib, p = _lib.load(), _lib.ptr
    res = {"device": torch.cuda.get_device_name(0), "rep": a.rep, "fit_steps": a.fit, "fit_l1": round(loss, 5), "cases": []}
    for n in (int(s) for s in a.sizes.split(",")):
        values, org, spc = sdf_grid(sdf, n)
        N = n ** 3
        ws_bytes = lib.iso_meshextract_workspace_bytes(n, n, n)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        totals = torch.empty((2,), dtype=torch.int64, device=dev)
        _lib.call("iso_meshextract_count", p(values), n, n, n, 0.0, p(totals), p(ws), ws_bytes, _lib.stream())
        V, F = totals.tolist()
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        cnt = torch.zeros((2 * N,), dtype=torch.int32, device=dev)
        off = torch.empty_like(cnt)
        scan_bytes = lib.iso_prefix_sum_workspace_bytes(N, 2)
        scan_ws = torch.empty((scan_bytes,), dtype=torch.uint8, device=dev)
        c = {"n": n, "points": N, "verts": V, "faces": F, "workspace_MB": round(ws_bytes / 1e6, 1)}
        c["sdf_grid_ms"] = timed(lambda: sdf_grid(sdf, n), a.rep)
        c["count_ms"] = timed(lambda: _lib.call("iso_meshextract_count", p(values), n, n, n, 0.0, p(totals), p(ws), ws_bytes,
                                                _lib.stream()), a.rep)
        c["scan_ms"] = timed(lambda: _lib.call("iso_prefix_sum", p(cnt), p(off), N, 2, N, p(scan_ws), scan_bytes,
                                               _lib.stream()), a.rep)
        c["emit_ms"] = timed(lambda: _lib.call("iso_meshextract_emit", p(values), n, n, n, org[0], org[1], org[2], spc[0],
                                               spc[1], spc[2], 0.0, p(totals), p(verts), V, p(faces), F, p(ws), ws_bytes,
                                               _lib.stream()), a.rep)
        c["call_ms"] = timed(lambda: marching_tetrahedra(values, org, spc), a.rep)
        classify = c["count_ms"][0] - c["scan_ms"][0]
        c["classify_ms"] = round(classify, 4)
        c["classify_volume_GBps"] = round(4 * N / classify / 1e6, 1)
        c["classify_traffic_GBps"] = round(13 * N / classify / 1e6, 1)
        # faster and different is not faster: the timed buffers hold what the public call returns
        v2, f2 = marching_tetrahedra(values, org, spc)
        assert torch.equal(v2, verts) and torch.equal(f2, faces.long())
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
        del values, ws, verts, faces, cnt, off, scan_ws, v2, f2
    print(json.dumps(res))


if __name__ == "__main__":
    main()
