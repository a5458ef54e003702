"""Plain numpy restatement of the N-rank exchange entries (csrc/band.hip, csrc/bricks_halo.hip) and the seeded case
generator that tests/test_exchange_cpu.py and tests/test_exchange_gpu.py share.  No GPU, no torch.

Everything the kernels do is data movement, integer selection and integer sums, so every comparison against this file
is exact.  The one piece of arithmetic -- which bands a row's bounding box touches -- is written statement for statement
in np.float32 (one rounding per operation, no contraction: the library is built with contraction off), so the mask
is the kernel's bit for bit, on boundaries too.  Float payloads travel as int32 bit patterns (NaNs travel)."""
import numpy as np

F32 = np.float32
TILE, REC, HDR, CHUNK = 16, 13, 16, 512
FIELDS = (("ndc", 3), ("ellipse", 3), ("radii", 2), ("scaler", 1), ("features", 3))     # the record's order on the wire
FLT_MAX = np.finfo(np.float32).max


# ----------------------------------------------------------------------------- frame, bands, the binning test
def make_frame(H, W=0):
    W = W if W > 0 else H
    m = min(H, W)
    return {"H": H, "W": W, "Tx": (W + 15) // 16, "Ty": (H + 15) // 16, "m": m, "ex": F32(W) / F32(m), "ey": F32(H) / F32(m)}


def band_of(d, world, Ty):
    """Tile rows [b, e) of rank d: dist.shard_bounds."""
    base, rem = divmod(Ty, world)
    b = d * base + min(d, rem)
    return b, b + base + (1 if d < rem else 0)


def pixel_range(c, r, n, e, m):
    """splat_frame.h::pixel_range on f32 arrays -> (ok, lo, hi)."""
    c, r, e = np.asarray(c, F32), np.asarray(r, F32), F32(e)
    with np.errstate(all="ignore"):
        ok = (r >= F32(0)) & (c == c)
        flo = ((c - r) + e) * F32(0.5) * F32(m) - F32(0.5)
        fhi = ((c + r) + e) * F32(0.5) * F32(m) - F32(0.5)
        ok &= flo < F32(1e9)
        ok &= fhi > F32(-1e9)
        flo = np.where(ok, np.maximum(flo, F32(-4.0)), F32(0))
        fhi = np.where(ok, np.minimum(fhi, F32(n) + F32(4.0)), F32(0))
        lo = np.ceil(flo).astype(np.int64) - 1
        hi = np.floor(fhi).astype(np.int64) + 1
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, n - 1)
    return ok & (lo <= hi), lo, hi


def band_mask(ndc, radii, frame, world):
    """band.hip::band_mask: uint64 per row, bit d = the binning pass of band d lists the row."""
    ndc, radii = np.asarray(ndc, F32).reshape(-1, 3), np.asarray(radii, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        ok = ndc[:, 2] >= F32(0)
    okx, _, _ = pixel_range(ndc[:, 0], radii[:, 0], frame["W"], frame["ex"], frame["m"])
    oky, y0, y1 = pixel_range(ndc[:, 1], radii[:, 1], frame["H"], frame["ey"], frame["m"])
    ok = ok & okx & oky
    t0, t1 = y0 // TILE, y1 // TILE
    m = np.zeros(ndc.shape[0], np.uint64)
    for d in range(world):
        b, e = band_of(d, world, frame["Ty"])
        m |= np.where(ok & (t0 < e) & (t1 >= b), np.uint64(1) << np.uint64(d), np.uint64(0))
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ----------------------------------------------------------------------------- the global layout
def global_layout(counts, world, n_views, rank=None):
    """first_global / num_global (n_views,) and, for `rank`, gid_first: view-major, ranks in order."""
    counts = np.asarray(counts, np.int64).reshape(world, 8)
    first_g, num_g, gid_first = np.zeros(n_views, np.int64), np.zeros(n_views, np.int64), np.zeros(n_views, np.int64)
    run = 0
    for v in range(n_views):
        first_g[v] = run
        for s in range(world):
            if s == rank:
                gid_first[v] = run
            run += int(counts[s, v])
        num_g[v] = run - first_g[v]
    return first_g, num_g, gid_first


def wire_records(rows, p, gid):
    """(len(p), 13) int32: the records of own rows p with global ids gid."""
    rec = np.empty((len(p), REC), np.int32)
    o = 0
    for name, w in FIELDS:
        rec[:, o:o + w] = bits(np.asarray(rows[name], F32).reshape(-1, w))[p]
        o += w
    rec[:, 12] = gid.astype(np.int32)
    return rec


# ----------------------------------------------------------------------------- band exchange
def export(rank_rows, counts, world, rank, frame, cap_pair):
    """iso_splat_band_export.  rank_rows: ndc / ellipse / radii / scaler / features (f32, packed own rows) + first / num
    (n_views int64).  Per destination d: headers[d] (16 int32), records[d] ((delivered, 13) int32 bit patterns, views
    ascending then row order), sent_row[d] (delivered,); flag; gid_first / first_global / num_global; own_rows: the rows
    whose acc / vis the call clears."""
    first, num = np.asarray(rank_rows["first"], np.int64), np.asarray(rank_rows["num"], np.int64)
    n_views = len(first)
    first_g, num_g, gid_first = global_layout(counts, world, n_views, rank)
    p_all = np.concatenate([first[v] + np.arange(num[v]) for v in range(n_views)] + [np.zeros(0, np.int64)]).astype(np.int64)
    g_all = np.concatenate([gid_first[v] + np.arange(num[v]) for v in range(n_views)] + [np.zeros(0, np.int64)]).astype(np.int64)
    v_all = np.concatenate([np.full(num[v], v) for v in range(n_views)] + [np.zeros(0, np.int64)]).astype(np.int64)
    mask = band_mask(np.asarray(rank_rows["ndc"], F32).reshape(-1, 3)[p_all], np.asarray(rank_rows["radii"], F32).reshape(-1, 2)[p_all],
                     frame, world)
    headers, records, sent_row, flag = np.zeros((world, HDR), np.int32), [], [], 0
    for d in range(world):
        sel = np.nonzero((mask >> np.uint64(d)) & np.uint64(1))[0]
        run = 0
        for v in range(8):
            c = int((v_all[sel] == v).sum()) if v < n_views else 0
            headers[d, v] = c if run + c <= cap_pair else max(cap_pair - run, 0)
            run += c
        headers[d, 8] = run
        if run > cap_pair:
            flag |= 1
        sel = sel[:min(run, cap_pair)]
        records.append(wire_records(rank_rows, p_all[sel], g_all[sel]))
        sent_row.append(p_all[sel].astype(np.int32))
    return {"headers": headers, "records": records, "sent_row": sent_row, "flag": flag, "gid_first": gid_first,
            "first_global": first_g, "num_global": num_g, "own_rows": p_all, "mask": mask, "gid": g_all}


def transpose(exports, d):
    """The all-to-all: what band d receives = segment d of every rank's export, as (header, records) per source."""
    return [(e["headers"][d], e["records"][d]) for e in exports]


def import_(segments, world, n_views, cap_pair, cap_local, cutoff):
    """iso_splat_band_import.  segments: per source rank (header (16,) int32, records (n, 13) int32)."""
    flag = 0
    for hdr, _ in segments:
        if int(hdr[8]) > cap_pair:
            flag = 2
    first_l, num_l = np.zeros(n_views, np.int64), np.zeros(n_views, np.int64)
    recs, origin = [], []
    run = 0
    for v in range(n_views):
        first_l[v] = run
        for s, (hdr, rec) in enumerate(segments):
            slot0, c = int(hdr[:v].sum()), int(hdr[v])
            if run + c > cap_local:
                c, flag = max(cap_local - run, 0), 2
            recs.append(rec[slot0:slot0 + c])
            origin.append(s * cap_pair + slot0 + np.arange(c))
            run += c
        num_l[v] = run - first_l[v]
    rec = np.concatenate(recs + [np.zeros((0, REC), np.int32)])
    out = {"first_local": first_l, "num_local": num_l, "flag": flag, "total": run, "gid": rec[:, 12].copy(),
           "origin": np.concatenate(origin + [np.zeros(0, np.int64)]).astype(np.int32),
           "cutoff": np.full(run, F32(cutoff), F32)}
    o = 0
    for name, w in FIELDS:
        out[name] = rec[:, o:o + w].copy()
        o += w
    return out


def remap(idx_local, gid, n_views, view_pixels, band_pixel0, band_pixels, K, idx_global):
    """iso_splat_band_remap on flat (n_views * view_pixels * K) arrays: the band's entries of every view."""
    out = np.array(idx_global, np.int32).reshape(-1).copy()
    idx_local = np.asarray(idx_local, np.int32).reshape(-1)
    for v in range(n_views):
        a = (v * view_pixels + band_pixel0) * K
        l = idx_local[a:a + band_pixels * K]
        out[a:a + band_pixels * K] = np.where(l >= 0, np.asarray(gid)[np.maximum(l, 0)], l)
    return out


def return_(acc_local, vis_local, origin, total, ret):
    """iso_splat_band_return: ret (world, cap_pair, 2) int64 (a copy with the slots of the local rows written)."""
    out = np.array(ret, np.int64).copy()
    flat = out.reshape(-1, 2)
    o = np.asarray(origin[:total], np.int64)
    flat[o, 0] = np.asarray(acc_local, np.int64)[:total]
    flat[o, 1] = np.asarray(vis_local)[:total]
    return out


def merge(back, sent_row, acc_own, vis_own):
    """iso_splat_band_merge: back (world, cap_pair, 2) int64 as it came back, sent_row: per band the own rows of the
    delivered records.  Sums wrap like the kernel's 64-bit adds."""
    acc = np.array(acc_own, np.int64).copy().view(np.uint64)
    vis = np.array(vis_own, np.uint8).copy()
    for d, rows in enumerate(sent_row):
        n = len(rows)
        np.add.at(acc, rows, np.asarray(back[d, :n, 0], np.int64).view(np.uint64))
        vis[rows[np.asarray(back[d, :n, 1]) != 0]] = 1
    return acc.view(np.int64), vis


def repack(blocks, capacity, world, rank, n_views, counts, cutoff, max_rows, out_rows, fill_bits):
    """iso_splat_repack.  blocks: (world, 12 * capacity) int32 bit patterns (ndc 3, ellipse 3, radii 2, scaler 1,
    features 3, each `capacity` rows).  Outputs hold out_rows rows pre-filled with fill_bits."""
    counts = np.asarray(counts, np.int64).reshape(world, 8)
    blocks = np.asarray(blocks, np.int32).reshape(world, 12 * capacity)
    at = {"ndc": 0, "ellipse": 3, "radii": 6, "scaler": 8, "features": 9}
    out = {name: np.full((out_rows, w), fill_bits, np.int32) for name, w in FIELDS}
    out["cutoff"] = np.full((out_rows,), fill_bits, np.int32)
    z = lambda: np.zeros(n_views, np.int64)                                        # noqa: E731
    first_g, num_g, own_first, own_num = z(), z(), z(), z()
    run = 0
    for v in range(n_views):
        first_g[v] = min(run, max_rows)
        for s in range(world):
            c = int(counts[s, v])
            if s == rank:
                own_first[v] = min(run, max_rows)
                own_num[v] = c if run + c <= max_rows else max(max_rows - run, 0)
            g0, l0, n = run, int(counts[s, :v].sum()), c
            if l0 + n > capacity:
                n = max(capacity - l0, 0)
            if g0 + n > max_rows:
                n = max(max_rows - g0, 0)
            for name, w in FIELDS:
                src = blocks[s, at[name] * capacity:(at[name] + w) * capacity].reshape(capacity, w) if capacity else None
                if n:
                    out[name][g0:g0 + n] = src[l0:l0 + n]
            out["cutoff"][g0:g0 + n] = bits(np.full(n, F32(cutoff), F32))
            run += c
        num_g[v] = min(run, max_rows) - first_g[v]
    out.update({"first_idx": first_g, "num_points": num_g, "own_first": own_first, "own_num": own_num})
    return out


# ----------------------------------------------------------------------------- halo exchange of the brick grid
def bk_fine(p, mn, inv_f, nf):
    """bricks.h::bk_fine on f32 arrays."""
    c = np.floor((np.asarray(p, F32) - F32(mn)) * F32(inv_f)).astype(np.int64)
    return np.clip(c, 0, nf - 1)


def halo_range(hdr, boxes, k, halo):
    lo = int(bk_fine(boxes[k][0], hdr["mn0"], hdr["inv_f"], hdr["nf0"])) - halo
    hi = int(bk_fine(boxes[k][4], hdr["mn0"], hdr["inv_f"], hdr["nf0"])) + halo
    return lo, hi


def halo_export_set(x_own, hdr, boxes, world, rank, halo):
    """Bool per own point: its fine x-cell lies in the widened range of some OTHER rank.  hdr: mn0, inv_f, nf0, f of the
    common header (f32 / int); boxes: (world, 8) f32."""
    fx = bk_fine(x_own, hdr["mn0"], hdr["inv_f"], hdr["nf0"])
    take = np.zeros(len(fx), bool)
    for k in range(world):
        if k != rank:
            lo, hi = halo_range(hdr, boxes, k, halo)
            take |= (fx >= lo) & (fx <= hi)
    return take


def halo_import_set(x_all, owner, exported, hdr, boxes, rank, halo):
    """Bool per point of the whole cloud: rank imports it (exported by another rank, fine x-cell in rank's widened
    range).  owner: rank per point; exported: bool per point (every rank's halo_export_set)."""
    lo, hi = halo_range(hdr, boxes, rank, halo)
    fx = bk_fine(x_all, hdr["mn0"], hdr["inv_f"], hdr["nf0"])
    return exported & (np.asarray(owner) != rank) & (fx >= lo) & (fx <= hi)


def halo_header_words(hdr, boxes, rank, halo):
    """(x_lo, x_hi) f32 and (own_bx_lo, own_bx_hi) int: words 28..31 of the header after iso_halo_import."""
    lo, hi = halo_range(hdr, boxes, rank, halo)
    mn, f, nf = F32(hdr["mn0"]), F32(hdr["f"]), hdr["nf0"]
    x_lo = F32(-FLT_MAX) if lo <= 0 else F32(mn + F32(lo) * f)
    x_hi = F32(FLT_MAX) if hi >= nf - 1 else F32(mn + F32(hi + 1) * f)
    return x_lo, x_hi, (lo + halo) >> 2, (hi - halo) >> 2


# ----------------------------------------------------------------------------- the case generator
SIZES = (0, 1, 511, 512, 513, 1025)                       # rows per view per rank; chunks are 512 rows


class Case(object):
    """One seeded exchange case: every rank's packed rows, the all-gathered counts and the capacities."""

    def __init__(self, cid, world, H, W, n_views, big=0, extra=0, cap="ample", seed=0):
        self.id, self.world, self.H, self.W, self.n_views, self.big, self.extra, self.cap = cid, world, H, W, n_views, big, extra, cap
        self.frame = make_frame(H, W)
        rng = np.random.default_rng(1000 * world + 10 * n_views + H + seed)
        self.empty_view = 1 if n_views >= 3 else -1          # no rank has a row of it
        self.single_view = 2 if n_views >= 3 else -1         # one rank only has rows of it
        self.counts = np.zeros((world, 8), np.int32)
        for r in range(world):
            for v in range(n_views):
                c = SIZES[(r + 2 * v + 3) % 6] if (r < 6 or world <= 10) else (r + v) % 2
                if v == self.empty_view or (v == self.single_view and r != min(1, world - 1)):
                    c = 0
                self.counts[r, v] = c
        if big:
            self.counts[world - 1, 0] = big                   # the second 64-chunk trip of k_band_scan
        self.max_rows = int(self.counts.max()) + extra
        self.rows = [self._rows(rng, self.counts[r, :n_views]) for r in range(world)]
        self._exports = None

    def _rows(self, rng, num):
        # views do not touch in the arrays (2 rows in front, 3 between views, rows like any other): what the entries clear
        # or send must follow first / num, not the array
        first = (np.concatenate([[0], np.cumsum(num)[:-1]]) + 2 + 3 * np.arange(len(num))).astype(np.int64)
        n, fr = int(num.sum()) + 2 + 3 * len(num), self.frame
        px = F32(2.0 / fr["m"])
        ndc = np.empty((n, 3), F32)
        ndc[:, 0] = rng.uniform(-1.3, 1.3, n) * fr["ex"]
        ndc[:, 1] = rng.uniform(-1.3, 1.3, n) * fr["ey"]
        ndc[:, 2] = rng.uniform(1e-3, 5.0, n)
        band_h = 2.0 * fr["ey"] / min(self.world, fr["Ty"])
        cls = rng.integers(0, 3, n)
        rad = np.where(cls == 0, rng.uniform(0.05, 0.9, n) * px, np.where(cls == 1, rng.uniform(0.3, 1.2, n) * band_h,
                                                                          rng.uniform(3.0, 6.0, n) * fr["ey"])).astype(F32)
        radii = np.stack([rad, (rad * rng.uniform(0.8, 1.25, n)).astype(F32)], 1).astype(F32)
        # fixed fractions of rows that no band may list, and the +inf radius that every band lists when the centre is sane
        kind = np.arange(n) % 40
        ndc[kind == 3, 2] = F32(-0.25)
        ndc[kind == 7, 0] = np.nan
        ndc[kind == 11, 2] = np.nan
        radii[kind == 13, 1] = F32(-1e-3)
        radii[kind == 17, 0] = np.nan
        radii[kind == 19] = np.inf
        ndc[kind == 23, 1] = F32(40.0)
        ndc[kind == 29, 1] = np.nan
        pay = lambda w: rng.integers(-2 ** 31, 2 ** 31, (n, w), dtype=np.int64).astype(np.int32).view(F32)   # noqa: E731
        ellipse, scaler, feat = pay(3), pay(1).reshape(n), pay(3)
        ellipse[n // 2, 0], feat[n // 2, 1], scaler[n // 2] = np.nan, F32(-0.0), F32(-0.0)
        return {"ndc": ndc, "ellipse": ellipse, "radii": radii, "scaler": scaler, "features": feat, "first": first,
                "num": np.asarray(num, np.int64)}

    # capacities follow from the unclipped exchange
    def exports(self, cap_pair=None):
        if cap_pair is None:
            if self._exports is None:
                self._exports = [export(self.rows[r], self.counts, self.world, r, self.frame, 1 << 40) for r in range(self.world)]
            return self._exports
        return [export(self.rows[r], self.counts, self.world, r, self.frame, cap_pair) for r in range(self.world)]

    def capacities(self):
        """(cap_pair, cap_local) of the case's capacity mode."""
        ex = self.exports()
        wanted = np.stack([e["headers"][:, 8] for e in ex])                     # (source, destination)
        largest = int(wanted.max())
        received = int(wanted.sum(0).max())
        cap_pair, cap_local = largest + 37, received + 41
        if self.cap == "pair_exact":
            cap_pair = largest
        elif self.cap == "pair_minus1":
            cap_pair = largest - 1
        elif self.cap == "pair_mid":                       # inside view 0 of the largest segment: later views get count 0
            s, d = np.unravel_index(int(wanted.argmax()), wanted.shape)
            cap_pair = int(ex[s]["headers"][d, 0]) // 2 + 1
        elif self.cap == "pair_zero":
            cap_pair = 0
        elif self.cap == "local_clip":
            cap_local = received // 2 + 1
        return cap_pair, cap_local

    def global_rows(self):
        """The single-GPU packed arrays: view-major, ranks in order."""
        out = {}
        for name, w in FIELDS:
            parts = []
            for v in range(self.n_views):
                for r in range(self.world):
                    a = self.rows[r]
                    parts.append(np.asarray(a[name]).reshape(-1, w)[a["first"][v]:a["first"][v] + a["num"][v]])
            out[name] = np.concatenate(parts)
        return out


def front_block(rows, capacity):
    """One rank's block of the all-gather form (12 * capacity int32 bit patterns): the rank's rows of every view packed from
    row 0, as iso_splat_front leaves them in one buffer (ndc 3, ellipse 3, radii 2, scaler 1, features 3)."""
    p = np.concatenate([rows["first"][v] + np.arange(rows["num"][v]) for v in range(len(rows["num"]))]).astype(np.int64)
    p = p[:capacity]
    blk = np.zeros(12 * capacity, np.int32)
    for name, at in (("ndc", 0), ("ellipse", 3), ("radii", 6), ("scaler", 8), ("features", 9)):
        a = bits(np.asarray(rows[name], F32).reshape(len(rows["scaler"]), -1)[p]).reshape(-1)
        blk[at * capacity:at * capacity + a.size] = a
    return blk


def _specs():
    views = {1: 1, 2: 3, 8: 8, 9: 3, 10: 8, 18: 1, 19: 3, 28: 3, 64: 8}
    out = []
    for k, w in enumerate((1, 2, 8, 9, 10, 18, 19, 28, 64)):
        out.append(dict(cid="w%d-1024-v%d" % (w, views[w]), world=w, H=1024, W=0, n_views=views[w], extra=1000 * (k % 2)))
    out.append(dict(cid="w9-64-v3-emptybands", world=9, H=64, W=0, n_views=3))
    out.append(dict(cid="w64-64-v8-emptybands", world=64, H=64, W=0, n_views=8, extra=1000))
    out.append(dict(cid="w5-130x67-v3", world=5, H=130, W=67, n_views=3))
    out.append(dict(cid="w2-1024-v3-33000", world=2, H=1024, W=0, n_views=3, big=33000))
    out.append(dict(cid="w9-1024-v3-33000", world=9, H=1024, W=0, n_views=3, big=33000, extra=1000))
    for w, nv in ((3, 3), (10, 8)):
        for cap in ("ample", "pair_exact", "pair_minus1", "pair_mid", "pair_zero", "local_clip"):
            out.append(dict(cid="w%d-1024-v%d-%s" % (w, nv, cap), world=w, H=1024, W=0, n_views=nv, cap=cap, seed=5))
        out.append(dict(cid="w%d-1024-v%d-ample-max+1000" % (w, nv), world=w, H=1024, W=0, n_views=nv, extra=1000, seed=5))
    return out


SPECS = _specs()
CASE_IDS = [s["cid"] for s in SPECS]
_CASES = {}


def case(cid):
    """The case of that id, built once and shared (tests must leave it unchanged)."""
    if cid not in _CASES:
        _CASES[cid] = Case(**[s for s in SPECS if s["cid"] == cid][0])
    return _CASES[cid]


def sphere_cloud_x(n, seed):
    """n points of a unit sphere in x-slab order (ascending x), f32."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p = p.astype(F32)
    return np.ascontiguousarray(p[np.argsort(p[:, 0], kind="stable")])
