"""The exchange oracle (tests/exchange_oracle.py) against itself, without a GPU: what tests/test_exchange_gpu.py compares
the band / repack / halo entries with must itself deliver every row to exactly the bands that list it.  Plus the orphan
guard of the C ABI: every entry of include/isopoints.h is called by the package or named by a test."""
import os
import re

import numpy as np
import pytest

import exchange_oracle as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMPLE = [c for c in X.CASE_IDS if not re.search(r"pair_|local_clip", c)]


def _bit(mask, d):
    return ((mask >> np.uint64(d)) & np.uint64(1)).astype(bool)


def _global_mask(c):
    g = c.global_rows()
    return g, X.band_mask(g["ndc"], g["radii"], c.frame, c.world)


@pytest.mark.parametrize("cid", AMPLE)
def test_transpose_of_exports_delivers_each_band_its_rows(cid):
    c = X.case(cid)
    g, gmask = _global_mask(c)
    first_g, num_g, _ = X.global_layout(c.counts, c.world, c.n_views)
    ex = c.exports()
    for e in ex:
        assert e["flag"] == 0 and np.array_equal(e["first_global"], first_g) and np.array_equal(e["num_global"], num_g)
    for d in range(c.world):
        got = X.import_(X.transpose(ex, d), c.world, c.n_views, 1 << 40, 1 << 40, 0.5)
        assert got["flag"] == 0
        for v in range(c.n_views):
            want = first_g[v] + np.nonzero(_bit(gmask[first_g[v]:first_g[v] + num_g[v]], d))[0]
            have = got["gid"][got["first_local"][v]:got["first_local"][v] + got["num_local"][v]]
            assert np.array_equal(have, want), (cid, d, v)                  # ascending global id inside a view
        for name, _w in X.FIELDS:
            assert np.array_equal(got[name], X.bits(g[name]).reshape(len(gmask), -1)[got["gid"]]), (cid, d, name)


@pytest.mark.parametrize("cid", ["w1-1024-v1", "w3-1024-v3-ample", "w10-1024-v8-ample", "w64-64-v8-emptybands"])
def test_repack_gives_the_global_layout(cid):
    c = X.case(cid)
    g = c.global_rows()
    cap = int(c.counts[:, :c.n_views].sum(1).max())
    blocks = np.stack([X.front_block(rows, cap) for rows in c.rows])
    total = int(c.counts.sum())
    first_g, num_g, gid_first = X.global_layout(c.counts, c.world, c.n_views, c.world - 1)
    out = X.repack(blocks, cap, c.world, c.world - 1, c.n_views, c.counts, 0.25, total, total + 3, 0x7fc0dead)
    assert np.array_equal(out["first_idx"], first_g) and np.array_equal(out["num_points"], num_g)
    assert np.array_equal(out["own_first"], gid_first) and np.array_equal(out["own_num"], c.counts[c.world - 1, :c.n_views])
    for name, w in X.FIELDS:
        assert np.array_equal(out[name][:total], X.bits(g[name]).reshape(total, w)), name
        assert (out[name][total:] == 0x7fc0dead).all()
    assert np.array_equal(out["cutoff"][:total], X.bits(np.full(total, 0.25, np.float32)))


@pytest.mark.parametrize("cid", ["w3-1024-v3-ample", "w10-1024-v8-ample", "w64-1024-v8", "w9-64-v3-emptybands"])
def test_return_then_merge_of_ones_is_the_popcount(cid):
    c = X.case(cid)
    ex = c.exports()
    cap_pair = int(max(e["headers"][:, 8].max() for e in ex)) + 1
    rets = []
    for d in range(c.world):
        got = X.import_(X.transpose(ex, d), c.world, c.n_views, cap_pair, 1 << 40, 0.5)
        n = got["total"]
        rets.append(X.return_(np.ones(n, np.int64), np.ones(n, np.uint8), got["origin"], n, np.zeros((c.world, cap_pair, 2), np.int64)))
    seen_all = False
    for r in range(c.world):
        back = np.stack([rets[d][r] for d in range(c.world)])                # the reverse all-to-all
        n_rows = len(c.rows[r]["scaler"])
        acc, vis = X.merge(back, ex[r]["sent_row"], np.zeros(n_rows, np.int64), np.zeros(n_rows, np.uint8))
        pop = np.array([bin(int(m)).count("1") for m in ex[r]["mask"]], np.int64)
        assert np.array_equal(acc[ex[r]["own_rows"]], pop) and np.array_equal(vis[ex[r]["own_rows"]], (pop > 0).astype(np.uint8))
        seen_all |= bool((pop == min(c.world, c.frame["Ty"])).any())
    assert seen_all                                                          # rows that every (non-empty) band lists exist


@pytest.mark.parametrize("cid", ["w9-64-v3-emptybands", "w64-64-v8-emptybands"])
def test_an_empty_band_receives_nothing(cid):
    c = X.case(cid)
    assert c.world > c.frame["Ty"]
    wanted = np.stack([e["headers"][:, 8] for e in c.exports()])
    for d in range(c.world):
        b, e = X.band_of(d, c.world, c.frame["Ty"])
        assert (wanted[:, d].sum() == 0) == (b == e), (d, b, e)


def test_band_of_is_shard_bounds():
    from iso_points_amd.dist import shard_bounds
    for ty in (1, 4, 5, 9, 64):
        for world in (1, 2, 3, 9, 10, 64):
            assert [X.band_of(d, world, ty) for d in range(world)] == [shard_bounds(ty, world, d) for d in range(world)]


@pytest.mark.parametrize("cid", X.CASE_IDS)
def test_cases_reach_what_they_are_for(cid):
    """The generator's own promises: rows no band lists, rows every band lists, an empty view, a view on one rank, and the
    capacity modes cutting where their names say."""
    c = X.case(cid)
    masks = np.concatenate([e["mask"] for e in c.exports()])
    assert (masks == 0).any() and (masks == np.uint64((1 << min(c.world, c.frame["Ty"])) - 1)).any()
    if c.n_views >= 3:
        assert c.counts[:, c.empty_view].sum() == 0 and (c.counts[:, c.single_view] > 0).sum() == 1
    cap_pair, cap_local = c.capacities()
    ex = c.exports(cap_pair)
    flags = [e["flag"] for e in ex]
    imps = [X.import_(X.transpose(ex, d), c.world, c.n_views, cap_pair, cap_local, 0.5) for d in range(c.world)]
    if c.cap in ("ample", "pair_exact"):
        assert not any(flags) and not any(i["flag"] for i in imps)
        if c.cap == "pair_exact":
            assert max(int(e["headers"][:, 8].max()) for e in ex) == cap_pair
    if c.cap == "pair_minus1":
        assert any(flags) and max(int(e["headers"][:, 8].max()) for e in ex) == cap_pair + 1
    if c.cap == "pair_mid":                                                  # the cut inside a view, later views count 0
        h = np.concatenate([e["headers"] for e in ex])
        cut = h[(h[:, 0] == cap_pair) & (h[:, 8] > cap_pair)]
        assert len(cut) and (cut[:, 1:8] == 0).all() and 0 < cap_pair
    if c.cap == "pair_zero":
        assert cap_pair == 0 and all(len(r) == 0 for e in ex for r in e["records"])
    if c.cap == "local_clip":                                                # inside a view of some band
        assert not any(flags) and any(i["flag"] == 2 and 0 < i["num_local"][i["num_local"] > 0][-1] and i["total"] == cap_local
                                      for i in imps)
        wanted = np.stack([e["headers"][:, :8] for e in ex]).sum(0)          # (destination, view) unclipped
        assert any(0 < i["num_local"][v] < wanted[d, v] for d, i in enumerate(imps) for v in range(c.n_views))


# ----------------------------------------------------------------------------- the C ABI's orphan guard
def _declared():
    text = open(os.path.join(ROOT, "include", "isopoints.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return sorted(set(re.findall(r"\b(iso_[a-z0-9_]+)\s*\(", text)))


def _orphans():
    """Entries of include/isopoints.h that nothing under iso_points_amd/ calls (the ctypes table of _lib.py does not count)
    and no file under tests/ names (this file and the oracle's prose do not count)."""
    pkg = []
    for dirpath, _dirs, files in os.walk(os.path.join(ROOT, "iso_points_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                if f == "_lib.py":
                    src = re.sub(r"SIGNATURES = \{.*?\n\}\n", "", src, flags=re.S)
                pkg.append(src)
    own = (os.path.basename(__file__), "exchange_oracle.py")
    tests = [open(os.path.join(ROOT, "tests", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "tests")))
             if f.endswith(".py") and f not in own]
    everything = "\n".join(pkg + tests)
    return [name for name in _declared() if not re.search(r"\b%s\b" % name, everything)]


def test_every_entry_of_the_header_is_called_or_tested():
    names = _declared()
    assert len(names) > 100 and "iso_splat_band_export" in names and "iso_halo_import" in names
    from iso_points_amd import _lib
    assert sorted(_lib.SIGNATURES) == names                                  # the table lists exactly the header
    assert _orphans() == [], "entries that nothing calls and no test names"
