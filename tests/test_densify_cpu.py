"""tests/densify_oracle.py pinned without a GPU:

  * it reproduces the reference's own fixtures (upsample_*.npz, insert.npz, ear_*.npz) where they carry what the oracle
    produces -- the points a round inserts are the candidates of its sparsest fathers, the children of insert;
  * it agrees with oracle/iso_oracle.py's upsample, ear_upsample, insert and repulsion_step on seeded inputs;
  * a float32 restatement of each kernel (same operations in the same order, torch float32) passes every criterion on
    every input set of tests/test_densify_gpu.py: the margins and the 1 % fence cap can be met by a correct float32
    implementation, and the exact cases are exact;
  * deliberately wrong variants of the restatements fail.
"""
import pytest
import torch

import densify_oracle as D
from test_oracle_golden import EAR_CASES, load
from util import rel_err


def _O():
    from oracle import iso_oracle as O
    return O


# --------------------------------------------------------------------------------- float32 restatements of the kernels
def _dist32(d):
    return torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def f32_upsample(pts, knn, j_end=None, last=False):
    """k_upsample_candidates.  Wrong variants: j_end (the min over j stops early), last (last maximum)."""
    n, K = knn.shape[:2]
    mid = D.mids_f32(pts, knn)
    best, cand = torch.full((n,), -1.0), pts.clone()
    for k in range(K):
        mn = _dist32(mid[:, k, None, :] - knn[:, :j_end]).amin(dim=-1).clamp_max(3.0e38)
        take = (mn >= best) if last else (mn > best)
        best, cand = torch.where(take, mn, best), torch.where(take[:, None], mid[:, k], cand)
    return best, cand


def f32_ear(pts, nrm, knn, knn_n, sens, j_end=None, last=False):
    """k_ear_candidates."""
    n, K = knn.shape[:2]
    mid = D.mids_f32(pts, knn)
    best, cand = torch.full((n,), -float("inf")), pts.clone()
    for k in range(K):
        d = mid[:, k, None, :] - knn[:, :j_end]
        a = d * knn_n[:, k, None, :]
        v = _dist32(d) - ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
        mn = v.amin(dim=-1).abs()
        mn = torch.sqrt(torch.where(mn > 1.0e-17, mn, torch.full_like(mn, 1.0e-17)))
        u = knn_n[:, k]
        edge = 2.0 - ((nrm[:, 0] * u[:, 0] + nrm[:, 1] * u[:, 1]) + nrm[:, 2] * u[:, 2])
        if sens == 2.0:
            edge = edge * edge
        elif sens != 1.0:
            edge = torch.pow(edge, sens)
        val = edge * mn
        take = (val >= best) if last else (val > best)
        best, cand = torch.where(take, val, best), torch.where(take[:, None], mid[:, k], cand)
    return best, cand


def f32_repulse(pts, nrm, idx_view, stride, inv_sigma, first=0):
    """k_repulse; idx_view (n,K) is read with row stride `stride` from its first element, as the kernel reads it."""
    n, K = idx_view.shape
    p = pts[first:first + n]
    if K == 0:
        return p.clone()
    rows = torch.as_strided(idx_view, (n, K), (stride, 1))
    sw, m = torch.zeros(n), torch.zeros(n, 3)
    for k in range(K):
        j = rows[:, k]
        ok, js = j >= 0, j.clamp(min=0)
        u = nrm[js]
        un = torch.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        u = u / torch.where(un > 1e-12, un, torch.full_like(un, 1e-12))[:, None]
        d = p - pts[js]
        w = torch.exp(-((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * inv_sigma)
        w = torch.where(ok, w, torch.zeros_like(w))
        dn = (d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1]) + d[:, 2] * u[:, 2]
        sw = sw + w
        m = m + w[:, None] * (d - dn[:, None] * u)
    den = torch.where(sw < 1.0e-17, torch.full_like(sw, 1.0e-17), sw)            # iso_eps_denom of a sum of weights >= 0
    return p + (sw + 1.0)[:, None] * m / den[:, None]


def f32_fathers(pts, lens, refs, n_refs, params, le_lim=False, ge_zero=False):
    """k_insert_fathers.  Wrong variants: le_lim (<= at params[1]), ge_zero (d2 >= 0)."""
    B, P = pts.shape[:2]
    best = torch.full((B, P), float("inf"))
    for r in range(min(int(n_refs), 64)):
        d = pts - refs[r]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = torch.where(dd < best, dd, best)
    f = (best < params[0]) & ((best <= params[1]) if le_lim else (best < params[1])) & ((best >= 0) if ge_zero else (best > 0))
    if lens is not None:
        f = f & (torch.arange(P)[None, :] < lens.view(-1, 1))
    return f.to(torch.uint8)


def f32_children(pts, knn, father, rank, first, patch, n_rows, first_columns=False, skip_missing=False):
    """k_insert_children.  Wrong variants: first_columns (k0 = 0), skip_missing (a child of a missing neighbour is not written)."""
    B, P, K = knn.shape
    out = torch.full((n_rows, 3), D.SENTINEL)
    k0 = 0 if first_columns else K - patch
    for b in range(B):
        rows = father[b].bool().nonzero().reshape(-1)
        if rows.numel() == 0:
            continue
        nb = knn[b, rows, k0:k0 + patch]
        m = pts[b][nb.clamp(min=0)] * (nb >= 0)[..., None].float()
        c = 2.0 * pts[b, rows][:, None, :] / 3.0 + m / 3.0
        at = (int(first[b]) + (rank[b, rows] - 1) * patch)[:, None] + torch.arange(patch)[None, :]
        if skip_missing:
            at, c = at[nb >= 0], c[nb >= 0]
        out[at.reshape(-1)] = c.reshape(-1, 3)
    return out


# --------------------------------------------------------------------------------- the restatements on every input set
_SCORES = {}


def scores(op, kind, n, K, sens=1.0):
    """The float64 reference of a candidate case, computed once and shared."""
    key = (op, kind, n, K, sens)
    if key not in _SCORES:
        pts, nrm, knn, knn_n = D.candidate_inputs(kind, n, K)
        _SCORES[key] = D.upsample_scores(pts, knn) if op == "upsample" else D.ear_scores(pts, nrm, knn, knn_n, sens)
    return _SCORES[key]


@pytest.mark.parametrize("kind,n,K,exact", D.upsample_case_list())
def test_upsample_restatement_passes(kind, n, K, exact):
    pts, _, knn, _ = D.candidate_inputs(kind, n, K)
    sp, cand = f32_upsample(pts, knn)
    D.check_candidates(*scores("upsample", kind, n, K), pts, knn, sp, cand, exact=exact)


@pytest.mark.parametrize("kind,n,K,sens,exact", D.ear_case_list())
def test_ear_restatement_passes(kind, n, K, sens, exact):
    pts, nrm, knn, knn_n = D.candidate_inputs(kind, n, K)
    sp, cand = f32_ear(pts, nrm, knn, knn_n, sens)
    D.check_candidates(*scores("ear", kind, n, K, sens), pts, knn, sp, cand, exact=exact)


def test_equal_neighbours_score_zero():
    """neighbours that equal the point: float64 score 0, the candidate is the point up to the two roundings of
    (p + 2 p) / 3 (which is NOT always p in float32) and column 0 is chosen"""
    pts, _, knn, _ = D.candidate_inputs("equal", 1000, 16)
    score, err = scores("upsample", "equal", 1000, 16)
    assert float(score.abs().max()) < 1e-15
    sp, cand = f32_upsample(pts, knn)
    assert bool((D.chosen_columns(pts, knn, cand) == 0).all())
    assert float((cand - pts).abs().max()) <= 2 * D.U32 * float(pts.abs().max()) and float(sp.max()) <= float(err.max())


def test_lattice_rows_tie():
    """the tie lattice does tie: a good share of rows has its float64 maximum in several columns with DIFFERENT midpoints,
    and first and last maximum differ there"""
    for kind, n, K in D.LATTICE_CASES[2:4]:
        pts, nrm, knn, knn_n = D.candidate_inputs(kind, n, K)
        for score, _ in (scores("upsample", kind, n, K), scores("ear", kind, n, K, 2.0)):
            top = score == score.amax(dim=-1, keepdim=True)
            last = K - 1 - top.flip(-1).int().argmax(dim=-1)
            mid = D.mids_f32(pts, knn)
            differ = (mid[torch.arange(n), last] != mid[torch.arange(n), D.first_maximum(score)]).any(dim=-1)
            assert float(differ.float().mean()) > 0.03                # (tens of rows in a thousand)


def test_wrong_candidate_variants_fail():
    kind, n, K = D.LATTICE_CASES[2]
    pts, nrm, knn, knn_n = D.candidate_inputs(kind, n, K)
    with pytest.raises(AssertionError, match="first maximum"):
        D.check_candidates(*scores("upsample", kind, n, K), pts, knn, *f32_upsample(pts, knn, last=True), exact=True)
    with pytest.raises(AssertionError, match="first maximum"):
        D.check_candidates(*scores("ear", kind, n, K, 2.0), pts, knn, *f32_ear(pts, nrm, knn, knn_n, 2.0, last=True), exact=True)
    pts, nrm, knn, knn_n = D.candidate_inputs("jitter", 1000, 16)
    with pytest.raises(AssertionError):
        D.check_candidates(*scores("upsample", "jitter", 1000, 16), pts, knn, *f32_upsample(pts, knn, j_end=15))
    with pytest.raises(AssertionError):
        D.check_candidates(*scores("ear", "jitter", 1000, 16), pts, knn, *f32_ear(pts, nrm, knn, knn_n, 1.0, j_end=15))
    # a candidate that is no midpoint of its row (a reciprocal instead of the division, say) is refused as such
    sp, cand = f32_upsample(pts, knn)
    with pytest.raises(AssertionError, match="no float32 midpoint"):
        D.check_candidates(*scores("upsample", "jitter", 1000, 16), pts, knn, sp, cand * (1 + 2.0 ** -22))


def test_powf_allowance_is_the_measured_one():
    """A_POW = 2 x the largest relative error (in units of 2^-24) of the restatement's float32 pow against float64"""
    g = torch.Generator().manual_seed(0)
    x = 1 + 2 * torch.rand(4000000, generator=g)
    worst = max(float(((torch.pow(x, s).double() - torch.pow(x.double(), s)).abs() / torch.pow(x.double(), s)).max())
                for s in (0.5, 1.5, 2.5)) / D.U32
    print("float32 pow vs float64: %.3f u" % worst)
    assert 0.5 * D.A_POW * 0.9 <= worst <= 0.5 * D.A_POW * 1.001


def _repulse_case(P, n, first, K, inv_sigma):
    pts, nrm, idx, inv = D.repulse_inputs(P, K)
    if inv_sigma is not None:
        inv = torch.tensor([inv_sigma], dtype=torch.float32)
    view = idx[first:first + n, 1:]
    return pts, nrm, view, inv, D.repulse(pts, nrm, view, float(inv), first)


@pytest.mark.parametrize("P,n,first,K,inv_sigma", D.REPULSE_CASES)
def test_repulse_restatement_passes(P, n, first, K, inv_sigma):
    pts, nrm, view, inv, ref = _repulse_case(P, n, first, K, inv_sigma)
    still = D.check_repulse(pts, ref, f32_repulse(pts, nrm, view, K + 1, inv, first), first)
    move = (ref - pts[first:first + n].double()).abs().max()
    if inv_sigma is not None or K == 0 or n == 1:
        assert still == n                                              # underflowed weights, no neighbours: nothing moves
    else:
        assert 0 < still < n and float(move) > 1e-4                    # the degenerate rows, and a real move elsewhere
    D.check_repulse(pts, ref, f32_repulse(pts, nrm, view.contiguous(), K, inv, first), first)   # a packed list


def test_wrong_repulse_variants_fail():
    pts, nrm, view, inv, ref = _repulse_case(5000, 1000, 300, 8, None)
    with pytest.raises(AssertionError):                                # a row stride of K when the view is wider
        D.check_repulse(pts, ref, f32_repulse(pts, nrm, view, 8, inv, 300), 300)
    with pytest.raises(AssertionError):                                # first_point ignored
        D.check_repulse(pts, ref, f32_repulse(pts, nrm, view, 9, inv, 0), 300)
    moved = f32_repulse(pts, nrm, view, 9, inv, 300)
    still = ((ref - pts[300:1300].double()) == 0).all(dim=-1)
    moved[still.nonzero()[0]] += 1e-7                                  # a zero-move row that is not bit-equal
    with pytest.raises(AssertionError, match="came back changed"):
        D.check_repulse(pts, ref, moved, 300)


@pytest.mark.parametrize("P,lens,n_refs", D.FATHERS_CASES)
def test_fathers_restatement_passes(P, lens, n_refs):
    pts, ln, refs, nr, params = D.fathers_inputs(P, lens, n_refs)
    mask, d2, fenced = D.fathers(pts, ln, refs, nr, params)
    share = D.check_fathers(mask, fenced, f32_fathers(pts, ln, refs, nr, params))
    assert share <= 0.01
    if P > 200:
        assert 0.02 < float(mask.float().mean()) < 0.9 and bool((d2 == 0).any())
    if P > 200 and n_refs < 50:                                        # rows past n_refs must not count
        with pytest.raises(AssertionError):
            D.check_fathers(mask, fenced, f32_fathers(pts, ln, refs, 50, params))
    if lens is not None:                                               # nor rows past a cloud's length
        with pytest.raises(AssertionError):
            D.check_fathers(mask, fenced, f32_fathers(pts, None, refs, nr, params))
    with pytest.raises(AssertionError):
        D.check_fathers(mask, fenced, f32_fathers(pts, ln, refs, nr, params, ge_zero=True))


def test_fathers_dyadic_and_wrong_inequalities():
    for pts, refs, nr, params in D.fathers_dyadic():
        mask, d2, fenced = D.fathers(pts, None, refs, nr, params)
        assert D.check_fathers(mask, fenced, f32_fathers(pts, None, refs, nr, params), max_fenced=0) == 0
        lo = float(params.min())
        assert bool((d2 == lo).any()) and bool((d2 == 0).any())
        assert bool(((d2 < lo) & (d2 > lo * (1 - 2.0 ** -21))).any()) and bool(((d2 > lo) & (d2 < lo * (1 + 2.0 ** -21))).any())
        assert bool(mask.any()) and not bool(mask[d2 >= lo].any())
        with pytest.raises(AssertionError):
            D.check_fathers(mask, fenced, f32_fathers(pts, None, refs, nr, params, ge_zero=True), max_fenced=0)
        if float(params[1]) < float(params[0]):
            with pytest.raises(AssertionError):
                D.check_fathers(mask, fenced, f32_fathers(pts, None, refs, nr, params, le_lim=True), max_fenced=0)


@pytest.mark.parametrize("P,lens,K", D.CHILDREN_CASES)
def test_children_restatement_passes(P, lens, K):
    pts, knn, father, rank, first, n_rows = D.children_inputs(P, lens, K)
    ref = D.children(pts, knn, father, first, 8, n_rows)
    D.check_children(ref, f32_children(pts, knn, father, rank, first, 8, n_rows))
    if P > 200:
        with pytest.raises(AssertionError):
            D.check_children(ref, f32_children(pts, knn, father, rank, first, 8, n_rows, skip_missing=True))
        if K > 8:
            with pytest.raises(AssertionError):
                D.check_children(ref, f32_children(pts, knn, father, rank, first, 8, n_rows, first_columns=True))
        shifted = f32_children(pts, knn, father, rank, first - 1, 8, n_rows)       # one row early: a gap row is written
        with pytest.raises(AssertionError):
            D.check_children(ref, shifted)


# --------------------------------------------------------------------------------- the reference's fixtures
def _sorted_rows(x):
    for c in (2, 1, 0):
        x = x[x[:, c].sort(stable=True).indices]
    return x


def _round_rows(score, mid32, n_new, max_P):
    """The rows one upsample round inserts (point_processing.py:340-352): the first-maximum candidates of the n_new
    fathers with the sparsest edge.  As a set, in lexicographic order: the reference orders them by its float32
    sparsity, which two near-equal fathers may swap against the float64 one."""
    col = D.first_maximum(score)
    cand = mid32[torch.arange(score.shape[0]), col]
    return _sorted_rows(cand[score.amax(dim=-1).sort().indices[-max_P:]][max_P - n_new:])


@pytest.mark.parametrize("name", ["upsample_K16.npz", "upsample_K31.npz", "upsample_batch.npz"])
def test_upsample_fixture_first_round(name):
    O = _O()
    g = load(name)
    pts, K = g["points"], int(g["K"])
    B, P = pts.shape[:2]
    lens = g["num_points"] if "num_points" in g else torch.full((B,), P, dtype=torch.long)
    want = g["n_points"] if torch.is_tensor(g["n_points"]) else torch.full((B,), int(g["n_points"]))
    knn = O.knn_points(pts, pts, lens, lens, K=K + 1, return_nn=True).knn[..., 1:, :]
    for b in range(B):
        n_new = min(int(want[b] - lens[b]), P // 8)
        if n_new <= 0:
            continue
        score, _ = D.upsample_scores(pts[b], knn[b])
        rows = _round_rows(score, D.mids_f32(pts[b], knn[b]), n_new, P // 8)
        # every round prepends its rows, so the first round's sit right before the input points (a cloud that is already
        # full still gets a later round's max_P rows in front, point_processing.py:352: search, do not count)
        out_b, L = g["out_points"][b], int(lens[b])
        end = next(s for s in range(out_b.shape[0] - L + 1) if torch.equal(out_b[s:s + L], pts[b, :L]))
        got = _sorted_rows(g["out_points"][b, end - n_new:end])
        assert torch.equal(rows, got), "%d of %d rows differ" % (int((rows != got).any(-1).sum()), n_new)


def _ear_first_round(O, out, P, idx, normals, sens):
    """the rows EdgeAwareProjection.upsample inserts first (:601-640), from the LOP-moved points out[-P:]"""
    moved = out[:, -P:]
    knn, knn_n = O.knn_gather(moved, idx)[0], O.knn_gather(normals, idx)[0]
    score, _ = D.ear_scores(moved[0], normals[0], knn, knn_n, sens)
    n_new = min(out.shape[1] - P, P // 10)
    return _round_rows(score, D.mids_f32(moved[0], knn), n_new, P // 10), _sorted_rows(out[0, -P - n_new:-P])


def test_ear_fixture_first_round():
    import math
    O = _O()
    for tag, kw in EAR_CASES.items():
        g = load("ear_%s.npz" % tag)
        P = g["points"].shape[1]
        num = torch.tensor([P])
        tree = O.ear_tree(g["points"], num, kw["knn_k"])
        _, nrm = O.compute_sdf_and_grad(g["points"], O.BoxSDF())
        nrm = torch.nn.functional.normalize(nrm, dim=-1, eps=1e-15)
        nrm, _, _ = O.ear_denoise_normals(g["points"], nrm, num, tree, 1 - math.cos(kw.get("sharpness_angle", 15) / 180 * math.pi))
        rows, got = _ear_first_round(O, g["out_points"], P, tree.idx, nrm, kw.get("edge_sensitivity", 1))
        assert torch.equal(rows, got), "%s: %d of %d rows differ" % (tag, int((rows != got).any(-1).sum()), rows.shape[0])


def test_insert_fixture():
    O = _O()
    g = load("insert.npz")
    P = g["points"].shape[1]
    r = D.insert(g["ref_points"], g["ref_metrics"], g["points"], torch.tensor([P]), O.frnn_grid_points)
    assert r["sizes"] == g["child_per_batch"].tolist() and float(r["fenced"].float().mean()) == 0
    assert rel_err(r["children"][0], g["child_pts"][0]) < 1e-6


# --------------------------------------------------------------------------------- oracle/iso_oracle.py on seeded inputs
def test_agrees_with_iso_oracle_upsample():
    O = _O()
    g = torch.Generator().manual_seed(2)
    pts = torch.rand(2, 300, 3, generator=g)
    lens = torch.tensor([300, 211])
    pts[1, 211:] = 0
    up, num = O.upsample(pts, torch.tensor([330, 230]), num_points=lens, neighborhood_size=12)
    knn = O.knn_points(pts, pts, lens, lens, K=13, return_nn=True).knn[..., 1:, :]
    for b, n_new in enumerate((30, 19)):
        score, _ = D.upsample_scores(pts[b], knn[b])
        assert torch.equal(_round_rows(score, D.mids_f32(pts[b], knn[b]), n_new, 300 // 8), _sorted_rows(up[b, :n_new]))


def test_agrees_with_iso_oracle_ear_upsample():
    O = _O()
    g = torch.Generator().manual_seed(3)
    P = 500
    pts = torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1)
    num = torch.tensor([P])
    for sens in (1, 2, 1.5):
        up, n = O.ear_upsample(pts, P, O.SphereSDF(), num.clone(), knn_k=12, upsample_ratio=1.08, edge_sensitivity=sens)
        assert int(n) == 540
        tree = O.ear_tree(pts, num, 12)
        nrm, _, _ = O.ear_denoise_normals(pts, pts.clone(), num, tree, 1 - __import__("math").cos(15 / 180 * 3.141592653589793))
        rows, got = _ear_first_round(O, up, P, tree.idx, nrm, sens)
        assert rows.shape[0] == 40 and torch.equal(rows, got)


def test_agrees_with_iso_oracle_insert_and_repulsion():
    O = _O()
    ref_p, ref_m, points, lens = D.insert_inputs()
    r = D.insert(ref_p, ref_m, points, lens, O.frnn_grid_points)
    assert float(r["fenced"].float().mean()) == 0 and r["sizes"][0] > 0 and r["sizes"][1] > 0 and r["sizes"][2] == 0
    child, cpb = O.insert(ref_p, ref_m, points, lens)
    assert cpb.tolist() == r["sizes"]
    for b in range(3):
        if r["sizes"][b]:
            assert rel_err(child[b, :r["sizes"][b]], r["children"][b]) < 1e-6
    pts, nrm, idx, inv = D.repulse_inputs(3000, 8)
    ref = D.repulse(pts, nrm, idx[:, 1:], float(inv))
    got = O.repulsion_step(pts[None], torch.nn.functional.normalize(nrm, dim=-1)[None], idx[None, :, 1:], inv)
    D.check_repulse(pts, ref, got[0])
