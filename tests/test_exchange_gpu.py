"""The N-rank exchange entries one by one, through the C ABI, against tests/exchange_oracle.py: iso_splat_band_export /
_import / _remap / _return / _merge, iso_splat_repack, iso_halo_export / _import (and iso_frnn_make_grid, the other entry
nothing launched).  All ranks of a case run in this process; the all-to-all is a transpose of the stacked send buffers, the
all-gather a torch.stack.  Every comparison is exact; every output is pre-filled with a sentinel and compared WHOLE, so a
write outside the documented extent fails too.

Which case runs which path (case ids of tests/exchange_oracle.py; export / import / return + merge take the same ids):

  path                                        band export, import, return + merge       the other entries
  ------------------------------------------  ----------------------------------------  ---------------------------------
  fast path (world <= 8: register counts)     w1-, w2-, w8-1024, w3-1024-v3-*, w5-130x67  remap: one path, test_band_remap
  LDS path of k_band_count (d >= 8)           w9-1024-v3 and every larger world          repack: one path, test_repack
  later rounds of k_band_fill (world > 9)     w10 (2), w18 / w19 (3), w28 (4), w64 (8)   halo: test_halo_export_import
  64-chunk trip of k_band_scan (> 32 768)     w2- / w9-1024-v3-33000                     --
  cap_pair clip (flag 1, prefix delivered)    w3 / w10 pair_minus1, pair_mid, pair_zero  repack: capacity_cut; halo: export
                                              (pair_exact: full and NOT flagged)         capacity, test_halo_capacities_too_small
  cap_local clip (flag 2, prefix delivered)   w3 / w10 local_clip                        repack: max_rows_cut; halo: import
                                                                                         capacity, test_halo_capacities_too_small
  empty bands (world > tile rows)             w9-64-v3-emptybands, w64-64-v8-emptybands  remap: band_pixels = 0; halo: a rank
                                                                                         that owns one point (single300)
  rows no band lists (z < 0, NaN, r < 0,      every case (a fixed fraction of its rows;  remap: -1 entries stay -1
  off-image), rows every band lists (r = inf) tests/test_exchange_cpu.py asserts both)
  more (destination, view) pairs than waves   w3-1024-v3 (9 pairs < 16) .. w64-v8 (512)
  of k_band_scan, > 64 header words"""
import numpy as np
import pytest
import torch

import exchange_oracle as X
from iso_points_amd import _lib, bricks

pytestmark = pytest.mark.gpu

SENT = 0x7fc0dead                      # int32 bit pattern of the sentinel (a NaN as f32)
SENT64 = 0x5eed5eed5eed5eed
call, ptr = _lib.call, _lib.ptr


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def filled(shape, dtype, dev, value=SENT):
    t = torch.empty(shape, dtype=dtype, device=dev)
    (t.view(torch.int32) if dtype == torch.float32 else t).fill_(value)
    return t


def host_bits(t):
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


# ----------------------------------------------------------------------------- one case through export and import
class Run(object):
    pass


_RUNS = {}


def export_rank(c, r, dev, cap_pair, counts_d, seg_floats, ws_bytes):
    rows = c.rows[r]
    n_alloc = rows["scaler"].shape[0]
    E = Run()
    E.rows = {k: up(rows[k], dev) for k in ("ndc", "ellipse", "radii", "scaler", "features", "first", "num")}
    E.send = filled((c.world, seg_floats), torch.float32, dev)
    E.sent_row = filled((c.world * cap_pair + 1,), torch.int32, dev)
    E.acc = filled((n_alloc,), torch.int64, dev, SENT64)
    E.vis = filled((n_alloc,), torch.uint8, dev, 0xAB)
    E.lay = filled((3, 8), torch.int64, dev, -7)
    E.flags = torch.zeros((1,), dtype=torch.int32, device=dev)
    E.ws = filled((ws_bytes,), torch.uint8, dev, 0xCD)            # (nothing in it needs to be zero on entry)

    def go():
        R = E.rows
        call("iso_splat_band_export", ptr(R["ndc"]), ptr(R["ellipse"]), ptr(R["radii"]), ptr(R["scaler"]), ptr(R["features"]),
             ptr(R["first"]), ptr(R["num"]), c.n_views, c.max_rows, ptr(counts_d), c.world, r, c.H, c.W, cap_pair,
             ptr(E.send), ptr(E.sent_row), ptr(E.acc), ptr(E.vis), ptr(E.lay[0]), ptr(E.lay[1]), ptr(E.lay[2]),
             ptr(E.flags), ptr(E.ws), ws_bytes, _lib.stream())
    E.go = go
    go()
    return E


def run_exchange(cid, dev):
    """Export on every rank, the transpose, import on every band: the device buffers and the oracle's results, once."""
    if cid in _RUNS:
        return _RUNS[cid]
    c, lib = X.case(cid), _lib.load()
    R = Run()
    R.c = c
    R.cap_pair, R.cap_local = c.capacities()
    R.seg_floats = lib.iso_splat_band_segment_floats(R.cap_pair)
    assert R.seg_floats == 16 + 13 * R.cap_pair
    R.ws_bytes = lib.iso_splat_band_export_workspace_bytes(c.max_rows, c.n_views, c.world)
    R.counts = up(c.counts, dev)
    R.exp = [export_rank(c, r, dev, R.cap_pair, R.counts, R.seg_floats, R.ws_bytes) for r in range(c.world)]
    R.want_exp = c.exports(R.cap_pair)
    recv_all = torch.stack([e.send for e in R.exp]).transpose(0, 1).contiguous()       # [d][s] = segment d of rank s
    R.imp = []
    cl = R.cap_local + 5
    for d in range(c.world):
        I = Run()
        I.recv = recv_all[d]
        I.f = {"ndc": filled((cl, 3), torch.float32, dev), "ellipse": filled((cl, 3), torch.float32, dev),
               "cutoff": filled((cl,), torch.float32, dev), "radii": filled((cl, 2), torch.float32, dev),
               "scaler": filled((cl,), torch.float32, dev), "features": filled((cl, 3), torch.float32, dev)}
        I.gid, I.origin = filled((cl,), torch.int32, dev), filled((cl,), torch.int32, dev)
        I.acc, I.vis = filled((cl,), torch.int64, dev, SENT64), filled((cl,), torch.uint8, dev, 0xAB)
        I.lay = filled((2, 8), torch.int64, dev, -7)
        I.place = filled((3 * c.world * c.n_views,), torch.int32, dev)
        I.flags = torch.zeros((1,), dtype=torch.int32, device=dev)
        call("iso_splat_band_import", ptr(I.recv), c.world, c.n_views, R.cap_pair, R.cap_local, 0.375, ptr(I.f["ndc"]),
             ptr(I.f["ellipse"]), ptr(I.f["cutoff"]), ptr(I.f["radii"]), ptr(I.f["scaler"]), ptr(I.f["features"]), ptr(I.gid),
             ptr(I.origin), ptr(I.acc), ptr(I.vis), ptr(I.lay[0]), ptr(I.lay[1]), ptr(I.place), ptr(I.flags), _lib.stream())
        R.imp.append(I)
    R.want_imp = [X.import_(X.transpose(R.want_exp, d), c.world, c.n_views, R.cap_pair, R.cap_local, 0.375) for d in range(c.world)]
    _RUNS[cid] = R
    return R


def expected_send(c, want, cap_pair, seg_floats):
    send = np.full((c.world, seg_floats), SENT, np.int32)
    sent_row = np.full((c.world * cap_pair + 1,), SENT, np.int32)
    for d in range(c.world):
        n = len(want["records"][d])
        send[d, :16] = want["headers"][d]
        send[d, 16:16 + 13 * n] = want["records"][d].reshape(-1)
        sent_row[d * cap_pair:d * cap_pair + n] = want["sent_row"][d]
    return send, sent_row


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_band_export(dev, cid):
    R = run_exchange(cid, dev)
    c = R.c
    for r, (E, want) in enumerate(zip(R.exp, R.want_exp)):
        send, sent_row = expected_send(c, want, R.cap_pair, R.seg_floats)
        got = host_bits(E.send)
        assert np.array_equal(got[:, :16], send[:, :16]), (cid, r, "headers")
        assert np.array_equal(got, send), (cid, r, "records / beyond the count")
        assert np.array_equal(host_bits(E.sent_row), sent_row), (cid, r, "sent_row")
        assert int(E.flags.item()) == want["flag"], (cid, r)
        lay = np.full((3, 8), -7, np.int64)
        lay[0, :c.n_views], lay[1, :c.n_views], lay[2, :c.n_views] = want["gid_first"], want["first_global"], want["num_global"]
        assert np.array_equal(E.lay.cpu().numpy(), lay), (cid, r)
        acc, vis = np.full(E.acc.shape[0], SENT64, np.int64), np.full(E.vis.shape[0], 0xAB, np.uint8)
        acc[want["own_rows"]], vis[want["own_rows"]] = 0, 0
        assert np.array_equal(E.acc.cpu().numpy(), acc) and np.array_equal(E.vis.cpu().numpy(), vis), (cid, r, "acc / vis")


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_band_export_twice_on_one_workspace(dev, cid):
    R = run_exchange(cid, dev)
    for r in sorted({0, R.c.world // 2, R.c.world - 1}):
        E = R.exp[r]
        before = [t.clone() for t in (E.send.view(torch.int32), E.sent_row, E.acc, E.vis, E.lay, E.flags)]
        E.flags.zero_()
        E.go()
        for a, b in zip(before, (E.send.view(torch.int32), E.sent_row, E.acc, E.vis, E.lay, E.flags)):
            assert torch.equal(a, b), (cid, r)


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_band_import(dev, cid):
    R = run_exchange(cid, dev)
    c = R.c
    for d, (I, want) in enumerate(zip(R.imp, R.want_imp)):
        n = want["total"]
        assert n <= R.cap_local
        lay = np.full((2, 8), -7, np.int64)
        lay[0, :c.n_views], lay[1, :c.n_views] = want["first_local"], want["num_local"]
        assert np.array_equal(I.lay.cpu().numpy(), lay), (cid, d)
        assert int(I.flags.item()) == want["flag"], (cid, d)
        for name in ("ndc", "ellipse", "radii", "scaler", "features", "cutoff"):
            got = host_bits(I.f[name])
            exp = np.full(got.shape, SENT, np.int32)
            exp[:n] = X.bits(want[name]).reshape((n,) + got.shape[1:])
            assert np.array_equal(got, exp), (cid, d, name)                  # after a clip: exactly the oracle's prefix
        for name, t in (("gid", I.gid), ("origin", I.origin)):
            exp = np.full(t.shape[0], SENT, np.int32)
            exp[:n] = want[name]
            assert np.array_equal(t.cpu().numpy(), exp), (cid, d, name)
        acc, vis = np.full(I.acc.shape[0], SENT64, np.int64), np.full(I.vis.shape[0], 0xAB, np.uint8)
        acc[:n], vis[:n] = 0, 0
        assert np.array_equal(I.acc.cpu().numpy(), acc) and np.array_equal(I.vis.cpu().numpy(), vis), (cid, d)


@pytest.mark.parametrize("cid", ["w3-1024-v3-ample", "w10-1024-v8-ample"])
def test_every_band_bins_what_the_global_rows_bin(dev, cid):
    """The rasteriser's own test: iso_splat_bin_count over band d's tile rows counts the same on the global packed rows and
    on the rows band d imported -- no band misses a row its binning would list."""
    R = run_exchange(cid, dev)
    c, lib = R.c, _lib.load()
    g = c.global_rows()
    first_g, num_g, _ = X.global_layout(c.counts, c.world, c.n_views)
    g_ndc, g_rad, g_first, g_num = up(g["ndc"], dev), up(g["radii"], dev), up(first_g, dev), up(num_g, dev)
    T = lib.iso_splat_tiles_per_side(c.H)
    n_tiles = c.n_views * T * T
    total = 0
    for d in range(c.world):
        b, e = X.band_of(d, c.world, T)
        I = R.imp[d]
        cnt_g = torch.zeros((n_tiles + 1,), dtype=torch.int32, device=dev)
        cnt_l = torch.zeros((n_tiles + 1,), dtype=torch.int32, device=dev)
        call("iso_splat_bin_count", ptr(g_ndc), ptr(g_rad), ptr(g_first), ptr(g_num), c.n_views, int(num_g.max()), c.H, c.W,
             b, e, ptr(cnt_g), _lib.stream())
        call("iso_splat_bin_count", ptr(I.f["ndc"]), ptr(I.f["radii"]), ptr(I.lay[0]), ptr(I.lay[1]), c.n_views, R.cap_local,
             c.H, c.W, b, e, ptr(cnt_l), _lib.stream())
        assert torch.equal(cnt_g, cnt_l), (cid, d)
        total += int(cnt_g.sum().item())
    assert total > 0


# ----------------------------------------------------------------------------- remap
@pytest.mark.parametrize("K", [1, 8])
def test_band_remap(dev, K):
    rng = np.random.default_rng(K)
    N, H, W, n_local = 3, 37, 21, 500
    gid = rng.permutation(100000)[:n_local].astype(np.int32)
    idx_l = rng.integers(-1, n_local, (N, H, W, K)).astype(np.int32)
    idx_l[0, 5, 0, 0], idx_l[2, 20, 20, K - 1] = n_local - 1, 0
    gid_d, idx_d = up(gid, dev), up(idx_l, dev)
    for y0, y1, nv in ((0, H, N), (5, 21, N), (36, 37, N), (7, 7, N), (3, 9, 0), (0, 16, 1)):
        out = filled((N, H, W, K), torch.int32, dev)
        call("iso_splat_band_remap", ptr(idx_d), ptr(gid_d), nv, H * W, y0 * W, (y1 - y0) * W, K, ptr(out), _lib.stream())
        want = X.remap(idx_l, gid, nv, H * W, y0 * W, (y1 - y0) * W, K, np.full(idx_l.size, SENT, np.int32))
        got = out.cpu().numpy()
        assert np.array_equal(got.reshape(-1), want), (y0, y1, nv)
        if nv and y1 > y0:
            band = got[:nv, y0:y1]
            assert np.array_equal(band, np.where(idx_l[:nv, y0:y1] >= 0, gid[np.maximum(idx_l[:nv, y0:y1], 0)], -1))
            assert (got[:nv, :y0] == SENT).all() and (got[:nv, y1:] == SENT).all() and (got[nv:] == SENT).all()
        else:
            assert (got == SENT).all()                                       # band_pixels = 0, n_views = 0: nothing


# ----------------------------------------------------------------------------- return + merge
@pytest.mark.parametrize("cid", ["w3-1024-v3-ample", "w10-1024-v8-ample", "w3-1024-v3-pair_minus1", "w10-1024-v8-pair_minus1",
                                 "w3-1024-v3-pair_mid", "w10-1024-v8-pair_mid", "w3-1024-v3-local_clip",
                                 "w10-1024-v8-local_clip", "w64-1024-v8", "w9-64-v3-emptybands", "w2-1024-v3-33000"])
def test_band_return_and_merge(dev, cid):
    R = run_exchange(cid, dev)
    c, cap = R.c, R.cap_pair
    rng = np.random.default_rng(7)
    # a record the receiver dropped at cap_local has no slot written by iso_splat_band_return (include/isopoints.h): the
    # caller's `ret` is zero there, as dist.py keeps it; everywhere else the sentinel shows what the call left alone
    fill = 0 if c.cap == "local_clip" else SENT64
    rets, want_rets = [], []
    for d, (I, want) in enumerate(zip(R.imp, R.want_imp)):
        n, cl = want["total"], I.acc.shape[0]
        acc = rng.integers(-2 ** 63, 2 ** 63, cl, dtype=np.int64) >> rng.integers(0, 3, cl)      # up to |2^62| .. 2^63
        acc[rng.integers(0, 5, cl) == 0] = 0
        vis = rng.integers(0, 2, cl).astype(np.uint8)
        ret = filled((c.world * cap * 2 + 2,), torch.int64, dev, fill)
        acc_d, vis_d = up(acc, dev), up(vis, dev)
        call("iso_splat_band_return", ptr(acc_d), ptr(vis_d), ptr(I.origin), ptr(I.lay[0]), ptr(I.lay[1]), c.n_views,
             R.cap_local, ptr(ret), _lib.stream())
        w = X.return_(acc, vis, want["origin"], n, np.full((c.world, cap, 2), fill, np.int64))
        got = ret.cpu().numpy()
        assert np.array_equal(got[:-2].reshape(c.world, cap, 2), w) and (got[-2:] == fill).all(), (cid, d)
        rets.append(ret[:-2].view(c.world, cap, 2))
        want_rets.append(w)
    back_all = torch.stack(rets).transpose(0, 1).contiguous() if cap else None          # [owner][band]
    touched_by_many = 0
    for r, (E, want) in enumerate(zip(R.exp, R.want_exp)):
        acc0, vis0 = E.acc.cpu().numpy(), E.vis.cpu().numpy()                # zero over the own rows, garbage elsewhere
        acc_d, vis_d = E.acc.clone(), E.vis.clone()
        back = back_all[r] if cap else torch.zeros((2,), dtype=torch.int64, device=dev)
        call("iso_splat_band_merge", ptr(back), ptr(E.sent_row), c.world, c.n_views, c.max_rows, cap, ptr(acc_d), ptr(vis_d),
             ptr(E.ws), _lib.stream())
        wb = np.stack([want_rets[d][r] for d in range(c.world)])
        acc_w, vis_w = X.merge(wb, want["sent_row"], acc0, vis0)
        assert np.array_equal(acc_d.cpu().numpy(), acc_w), (cid, r, "acc_own")
        assert np.array_equal(vis_d.cpu().numpy(), vis_w), (cid, r, "vis_own")
        hits = np.zeros(len(acc0), np.int64)
        for rows in want["sent_row"]:
            np.add.at(hits, rows, 1)
        touched_by_many += int((hits > 1).sum())
    if c.cap != "pair_zero":
        assert touched_by_many > 0                                           # rows whose sums came from several bands


# ----------------------------------------------------------------------------- repack
@pytest.mark.parametrize("mode", ["ample", "capacity_cut", "max_rows_cut"])
@pytest.mark.parametrize("cid", ["w1-1024-v1", "w3-1024-v3-ample", "w10-1024-v8-ample"])
def test_repack(dev, cid, mode):
    c = X.case(cid)
    per_rank = c.counts[:, :c.n_views].sum(1)
    total = int(per_rank.sum())
    capacity = int(per_rank.max()) + (3 if mode != "capacity_cut" else -5)
    max_rows = total + 4 if mode != "max_rows_cut" else total - 100
    blocks = np.stack([X.front_block(rows, capacity) for rows in c.rows])
    blocks_d, counts_d = up(blocks, dev).view(torch.float32), up(c.counts, dev)
    out_rows = max_rows + 6
    for rank in sorted({0, c.world - 1}):
        o = {"ndc": filled((out_rows, 3), torch.float32, dev), "ellipse": filled((out_rows, 3), torch.float32, dev),
             "cutoff": filled((out_rows,), torch.float32, dev), "radii": filled((out_rows, 2), torch.float32, dev),
             "scaler": filled((out_rows, 1), torch.float32, dev), "features": filled((out_rows, 3), torch.float32, dev)}
        lay = filled((4, 8), torch.int64, dev, -7)
        call("iso_splat_repack", ptr(blocks_d), capacity, c.world, rank, c.n_views, ptr(counts_d), 0.375, max_rows,
             ptr(o["ndc"]), ptr(o["ellipse"]), ptr(o["cutoff"]), ptr(o["radii"]), ptr(o["scaler"]), ptr(o["features"]),
             ptr(lay[0]), ptr(lay[1]), ptr(lay[2]), ptr(lay[3]), _lib.stream())
        want = X.repack(blocks, capacity, c.world, rank, c.n_views, c.counts, 0.375, max_rows, out_rows, SENT)
        for name in o:
            assert np.array_equal(host_bits(o[name]).reshape(want[name].shape), want[name]), (cid, mode, rank, name)
        wl = np.full((4, 8), -7, np.int64)
        for k, name in enumerate(("first_idx", "num_points", "own_first", "own_num")):
            wl[k, :c.n_views] = want[name]
        assert np.array_equal(lay.cpu().numpy(), wl), (cid, mode, rank)
    if mode == "ample":                        # the all-gather form holds, at its global id, every row a band imported
        R = run_exchange(cid, dev)
        packed = {name: host_bits(o[name]).reshape(out_rows, -1) for name in o}
        for d, I in enumerate(R.imp):
            lay = I.lay.cpu().numpy()
            n = int(lay[0, c.n_views - 1] + lay[1, c.n_views - 1])
            assert n == R.want_imp[d]["total"], (cid, d)
            gid = I.gid.cpu().numpy()[:n]                    # (on the host: an id out of range fails here, not in a kernel)
            assert ((gid >= 0) & (gid < total)).all(), (cid, d)
            for name in packed:
                assert np.array_equal(packed[name][gid], host_bits(I.f[name]).reshape(I.acc.shape[0], -1)[:n]), (cid, d, name)


# ----------------------------------------------------------------------------- halo exchange of the brick grid
def _halo_cloud(kind, world):
    """(points in x-slab order, [lo, hi) of every rank)"""
    if kind == "sphere6000":
        pts = X.sphere_cloud_x(6000, 3)
        from iso_points_amd.dist import all_shard_bounds
        return pts, all_shard_bounds(6000, world)
    pts = X.sphere_cloud_x(300, 4)                                           # one rank owns a single point
    rest = 299
    cuts = [0, 1] + [1 + (rest * k) // (world - 1) for k in range(1, world)]
    return pts, [(cuts[k], cuts[k + 1]) for k in range(world)]


def _halo_run(dev, pts, bounds, halo, with_extras, capacity=None, import_capacity=None):
    world, P = len(bounds), len(pts)
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=(P, 3)).astype(np.float32)
    pay = rng.integers(-2 ** 31, 2 ** 31, P, dtype=np.int64).astype(np.int32)
    boxes = np.zeros((world, 8), np.float32)
    for k, (lo, hi) in enumerate(bounds):
        boxes[k, :3], boxes[k, 4:7] = pts[lo:hi].min(0), pts[lo:hi].max(0)
    boxes_d = up(boxes, dev)
    owner = np.concatenate([np.full(hi - lo, k) for k, (lo, hi) in enumerate(bounds)])
    cap = capacity if capacity is not None else max(hi - lo for lo, hi in bounds) + 3
    icap = import_capacity if import_capacity is not None else P
    grids, hdrs, bufs, exported = [], [], [], np.zeros(P, bool)
    for k, (lo, hi) in enumerate(bounds):
        g = bricks.BrickGrid(hi - lo, dev, import_max=P)
        call("iso_bricks_params", ptr(boxes_d), world, P, hi - lo, lo, -1.0, 8, 2.0, ptr(g.ws), g.n_max, _lib.stream())
        raw = g.ws[:128].cpu()
        f, i = raw.view(torch.float32).numpy(), raw.view(torch.int32).numpy()
        hdr = {"mn0": f[0], "inv_f": f[3], "f": f[8], "nf0": int(i[20])}
        assert int(i[25]) == lo and int(i[24]) == hi - lo
        buf = filled((2 * (cap + 1) * 4,), torch.float32, dev)
        p_d = up(pts[lo:hi], dev)
        n_d = up(nrm[lo:hi], dev) if with_extras else None
        y_d = up(pay[lo:hi], dev) if with_extras else None
        call("iso_halo_export", ptr(g.ws), ptr(p_d), ptr(n_d), ptr(y_d), hi - lo, ptr(boxes_d), world, k, halo, ptr(buf), cap,
             _lib.stream())
        take = X.halo_export_set(pts[lo:hi, 0], hdr, boxes, world, k, halo)
        exported[lo:hi] = take
        b = host_bits(buf).reshape(2, cap + 1, 4)
        n_rec = min(int(take.sum()), cap)
        assert int(b[0, 0, 0]) == int(take.sum()) and (b[0, 0, 1:] == 0).all(), (k, "count word, even above capacity")
        assert (b[1, 0] == SENT).all() and (b[0, 1 + n_rec:] == SENT).all() and (b[1, 1 + n_rec:] == SENT).all(), k
        rec0, rec1 = b[0, 1:1 + n_rec], b[1, 1:1 + n_rec]
        order = np.argsort(rec0[:, 3], kind="stable")
        ids = rec0[order, 3]
        assert len(np.unique(ids)) == n_rec and np.isin(ids, lo + np.nonzero(take)[0]).all(), k
        if n_rec == int(take.sum()):
            assert np.array_equal(ids, lo + np.nonzero(take)[0]), k
        assert np.array_equal(rec0[order, :3], X.bits(pts)[ids]), k
        assert np.array_equal(rec1[order, :3], X.bits(nrm)[ids] if with_extras else np.zeros((n_rec, 3), np.int32)), k
        assert np.array_equal(rec1[order, 3], pay[ids] if with_extras else np.zeros(n_rec, np.int32)), k
        grids.append(g), hdrs.append(hdr), bufs.append(buf)
    gathered = torch.stack(bufs)
    counts = [int(exported[lo:hi].sum()) for lo, hi in bounds]
    out = []
    for k, (lo, hi) in enumerate(bounds):
        g = grids[k]
        imp0, imp1 = filled((icap + 2, 4), torch.float32, dev), filled((icap + 2, 4), torch.float32, dev)
        cnt = filled((1,), torch.int32, dev)
        call("iso_halo_import", ptr(g.ws), g.n_max, ptr(gathered), ptr(boxes_d), world, k, halo, cap, ptr(imp0), ptr(imp1),
             ptr(cnt), icap, _lib.stream())
        want = np.nonzero(X.halo_import_set(pts[:, 0], owner, exported, hdrs[k], boxes, k, halo))[0]
        a0, a1, n_got = host_bits(imp0), host_bits(imp1), int(cnt.item())
        n_rec = min(n_got, icap)
        assert (a0[n_rec:] == SENT).all() and (a1[n_rec:] == SENT).all(), k
        order = np.argsort(a0[:n_rec, 3], kind="stable")
        ids = a0[order, 3]
        assert len(np.unique(ids)) == n_rec and np.isin(ids, want).all(), (k, "a duplicate-free subset of the oracle's set")
        assert np.array_equal(a0[order, :3], X.bits(pts)[ids]), k
        assert np.array_equal(a1[order, :3], X.bits(nrm)[ids] if with_extras else np.zeros((n_rec, 3), np.int32)), k
        assert np.array_equal(a1[order, 3], pay[ids] if with_extras else np.zeros(n_rec, np.int32)), k
        raw = g.ws[:128].cpu()
        x_lo, x_hi, bx_lo, bx_hi = X.halo_header_words(hdrs[k], boxes, k, halo)
        assert np.array_equal(raw.view(torch.int32).numpy()[28:30], X.bits(np.array([x_lo, x_hi], np.float32))), k
        assert raw.view(torch.int32).numpy()[30:32].tolist() == [bx_lo, bx_hi], k
        counters = g.ws[256:320].cpu().view(torch.int32).numpy()
        out.append({"want": want, "ids": ids, "count": n_got, "ovf_export": int(counters[4]), "ovf_import": int(counters[5]),
                    "sources_over": sum(1 for s in range(world) if s != k and counts[s] > cap)})
    return out, counts


@pytest.mark.parametrize("halo", [1, 2, 4])
@pytest.mark.parametrize("cloud", ["sphere6000", "single300"])
@pytest.mark.parametrize("world", [2, 3, 9])
def test_halo_export_import(dev, world, cloud, halo):
    pts, bounds = _halo_cloud(cloud, world)
    some = 0
    for with_extras in (True, False):
        out, counts = _halo_run(dev, pts, bounds, halo, with_extras)
        for k, o in enumerate(out):
            assert o["count"] == len(o["want"]) and np.array_equal(o["ids"], o["want"]), (k, "the imported set")
            assert o["ovf_export"] == 0 and o["ovf_import"] == 0, k
            some += len(o["want"])
    assert some > 0


@pytest.mark.parametrize("world", [2, 3, 9])
def test_halo_capacities_too_small(dev, world):
    pts, bounds = _halo_cloud("sphere6000", world)
    _, counts = _halo_run(dev, pts, bounds, 2, True)
    cap = sorted(counts)[-1] // 2                                            # below the largest export count
    out, _ = _halo_run(dev, pts, bounds, 2, True, capacity=cap)
    assert any(o["sources_over"] for o in out)
    for k, o in enumerate(out):
        assert o["ovf_export"] == o["sources_over"] and o["ovf_import"] == 0, k          # counters[4]: overflowing sources
        assert len(o["ids"]) <= len(o["want"])
    full, _ = _halo_run(dev, pts, bounds, 2, True)
    icap = max(len(o["want"]) for o in full) // 2
    out, _ = _halo_run(dev, pts, bounds, 2, True, import_capacity=icap)
    for k, o in enumerate(out):
        assert o["count"] == len(o["want"]), k
        assert o["ovf_import"] == max(len(o["want"]) - icap, 0) and o["ovf_export"] == 0, k   # counters[5]: the shortfall
    assert any(o["ovf_import"] for o in out)


# ----------------------------------------------------------------------------- refusals: they return before any launch
def test_refusals(dev):
    c = X.case("w3-1024-v3-ample")
    lib = _lib.load()
    rows = {k: up(c.rows[0][k], dev) for k in ("ndc", "ellipse", "radii", "scaler", "features", "first", "num")}
    cap = 64
    big = filled((65 * (16 + 13 * cap),), torch.float32, dev)
    sent_row, lay = filled((65 * cap,), torch.int32, dev), filled((3, 8), torch.int64, dev, -7)
    flags = torch.zeros((1,), dtype=torch.int32, device=dev)
    counts = torch.zeros((65, 8), dtype=torch.int32, device=dev)
    ws = filled((lib.iso_splat_band_export_workspace_bytes(c.max_rows, 8, 64) + 4096,), torch.uint8, dev, 0)

    def export(world=3, n_views=3, rank=0, ws_bytes=None):
        call("iso_splat_band_export", ptr(rows["ndc"]), ptr(rows["ellipse"]), ptr(rows["radii"]), ptr(rows["scaler"]),
             ptr(rows["features"]), ptr(rows["first"]), ptr(rows["num"]), n_views, c.max_rows, ptr(counts), world, rank, 1024, 0,
             cap, ptr(big), ptr(sent_row), None, None, ptr(lay[0]), ptr(lay[1]), ptr(lay[2]), ptr(flags), ptr(ws),
             ws.numel() if ws_bytes is None else ws_bytes, _lib.stream())
    for kw in (dict(world=65), dict(n_views=9), dict(rank=3), dict(world=64, rank=64),
               dict(ws_bytes=lib.iso_splat_band_export_workspace_bytes(c.max_rows, 3, 3) - 1)):
        with pytest.raises(RuntimeError):
            export(**kw)
    torch.cuda.synchronize()
    assert (host_bits(big) == SENT).all() and (sent_row.cpu().numpy() == SENT).all() and int(flags.item()) == 0
    pts, bounds = _halo_cloud("single300", 2)
    g = bricks.BrickGrid(1, dev, import_max=300)
    boxes = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    buf, imp, cnt = filled((2 * 301 * 4,), torch.float32, dev), filled((300, 4), torch.float32, dev), filled((1,), torch.int32, dev)
    with pytest.raises(RuntimeError):
        call("iso_halo_import", ptr(g.ws), g.n_max, ptr(torch.stack([buf, buf])), ptr(boxes), 2, 0, 0, 300, ptr(imp), ptr(imp),
             ptr(cnt), 300, _lib.stream())
    assert int(cnt.item()) == SENT


# ----------------------------------------------------------------------------- the other entry nothing launched
def test_frnn_make_grid_is_the_density_form_at_eight(dev):
    pts = up(X.sphere_cloud_x(300, 9).reshape(1, 300, 3), dev)
    lengths = torch.tensor([300], dtype=torch.int64, device=dev)
    radius = torch.tensor([0.2], dtype=torch.float32, device=dev)
    a, b = filled((1, 8), torch.float32, dev), filled((1, 8), torch.float32, dev)
    call("iso_frnn_make_grid", ptr(pts), ptr(lengths), ptr(radius), 1, 300, 128, ptr(a), _lib.stream())
    call("iso_frnn_make_grid_density", ptr(pts), ptr(lengths), ptr(radius), 1, 300, 128, 8.0, ptr(b), _lib.stream())
    assert np.array_equal(host_bits(a), host_bits(b)) and (host_bits(a) != SENT).all()
