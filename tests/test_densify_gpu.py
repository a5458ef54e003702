"""The densify stage's five kernels (csrc/repulse.hip, csrc/insert.hip) against tests/densify_oracle.py: float64, at
the K, launch and list edges -- partial last workgroups, the grid-stride second sweep (more than 4096 workgroups),
K from 1 to 64 (the EAR kernel's 96 KiB of LDS), strided and sharded index lists, degenerate rows, exact ties, and
the strict inequalities of the father mask.  The criteria and the input sets are the oracle's; test_densify_cpu.py shows
on the CPU that a correct float32 implementation meets them and that wrong ones do not."""
import pytest
import torch

import densify_oracle as D
from util import rel_err, sphere_cloud

pytestmark = pytest.mark.gpu

ISO_OK, ISO_ERR_INVALID = 0, -1


def _O():
    from oracle import iso_oracle as O
    return O


def _lib():
    from iso_points_amd import _lib
    return _lib


def _raw(name, *args):
    """the return code itself (_lib.call raises on a refusal)"""
    return getattr(_lib().load(), name)(*args)


# ----------------------------------------------------------------------------------------------- candidates
_REF = {}


def _candidate_case(op, kind, n, K, sens=1.0):
    """inputs and their float64 scores, computed once per case and left unchanged"""
    key = (op, kind, n, K, sens)
    if key not in _REF:
        inp = D.candidate_inputs(kind, n, K)
        _REF[key] = (inp, D.upsample_scores(inp[0], inp[2]) if op == "upsample" else D.ear_scores(*inp, sens))
    return _REF[key]


def _run_upsample(dev, pts, knn):
    L = _lib()
    n, K = knn.shape[:2]
    a, b = pts.to(dev).contiguous(), knn.to(dev).contiguous()
    sp = torch.full((n,), D.SENTINEL, device=dev)
    cand = torch.full((n, 3), D.SENTINEL, device=dev)
    L.call("iso_upsample_candidates", L.ptr(a), L.ptr(b), n, K, L.ptr(sp), L.ptr(cand), L.stream())
    return sp, cand


def _run_ear(dev, pts, nrm, knn, knn_n, sens):
    L = _lib()
    n, K = knn.shape[:2]
    a = [t.to(dev).contiguous() for t in (pts, nrm, knn, knn_n)]
    sp = torch.full((n,), D.SENTINEL, device=dev)
    cand = torch.full((n, 3), D.SENTINEL, device=dev)
    L.call("iso_ear_candidates", *[L.ptr(t) for t in a], n, K, float(sens), L.ptr(sp), L.ptr(cand), L.stream())
    return sp, cand


@pytest.mark.parametrize("kind,n,K,exact", D.upsample_case_list())
def test_upsample_candidates(dev, kind, n, K, exact):
    (pts, _, knn, _), (score, err) = _candidate_case("upsample", kind, n, K)
    sp, cand = _run_upsample(dev, pts, knn)
    D.check_candidates(score, err, pts, knn, sp, cand, exact=exact)
    sp2, cand2 = _run_upsample(dev, pts, knn)                                  # two identical calls: identical bits
    assert torch.equal(sp, sp2) and torch.equal(cand, cand2)


@pytest.mark.parametrize("kind,n,K,sens,exact", D.ear_case_list())
def test_ear_candidates(dev, kind, n, K, sens, exact):
    (pts, nrm, knn, knn_n), (score, err) = _candidate_case("ear", kind, n, K, sens)
    sp, cand = _run_ear(dev, pts, nrm, knn, knn_n, sens)
    D.check_candidates(score, err, pts, knn, sp, cand, exact=exact)
    sp2, cand2 = _run_ear(dev, pts, nrm, knn, knn_n, sens)
    assert torch.equal(sp, sp2) and torch.equal(cand, cand2)


def test_equal_neighbours(dev):
    """neighbours that equal the point: sparsity 0 up to the rounding of (p + 2 p) / 3, the candidate is column 0's
    midpoint -- the point to within those two roundings"""
    (pts, nrm, knn, knn_n), (_, err) = _candidate_case("upsample", "equal", 1000, 16)
    for sp, cand in (_run_upsample(dev, pts, knn), _run_ear(dev, pts, nrm, knn, knn_n, 1.0)):
        assert torch.equal(cand.cpu(), D.mids_f32(pts, knn)[:, 0])
        assert float((cand.cpu() - pts).abs().max()) <= 2 * D.U32 * float(pts.abs().max())
    assert float(_run_upsample(dev, pts, knn)[0].max()) <= float(err.max())


def test_candidates_no_stale_lds(dev):
    """a K = 64 call and then a K = 2 call on the same stream: the K = 2 result is the one the float64 reference accepts
    and the same bits as a K = 2 call made before any K = 64 one -- nothing of the wider call's LDS columns is read"""
    (p2, n2, k2, kn2), (s_u, e_u) = _candidate_case("upsample", "jitter", 1000, 2)
    (_, (s_e, e_e)) = _candidate_case("ear", "jitter", 1000, 2)
    before_u, before_e = _run_upsample(dev, p2, k2), _run_ear(dev, p2, n2, k2, kn2, 1.0)
    (p64, n64, k64, kn64), _ = _candidate_case("upsample", "jitter", 1000, 64)
    _run_upsample(dev, p64, k64)
    after_u = _run_upsample(dev, p2, k2)
    _run_ear(dev, p64, n64, k64, kn64, 1.0)
    after_e = _run_ear(dev, p2, n2, k2, kn2, 1.0)
    D.check_candidates(s_u, e_u, p2, k2, *after_u)
    D.check_candidates(s_e, e_e, p2, k2, *after_e)
    assert torch.equal(before_u[0], after_u[0]) and torch.equal(before_u[1], after_u[1])
    assert torch.equal(before_e[0], after_e[0]) and torch.equal(before_e[1], after_e[1])


def test_candidates_refusals(dev):
    """K = 0 and K = 65 are ISO_ERR_INVALID, n = 0 is ISO_OK; none of them writes"""
    L = _lib()
    n = 64
    pts, nrm = torch.rand(n, 3, device=dev), torch.rand(n, 3, device=dev)
    knn, knn_n = torch.rand(n, 65, 3, device=dev), torch.rand(n, 65, 3, device=dev)
    sp = torch.full((n,), D.SENTINEL, device=dev)
    cand = torch.full((n, 3), D.SENTINEL, device=dev)
    p = L.ptr
    for rows, K, want in ((n, 0, ISO_ERR_INVALID), (n, 65, ISO_ERR_INVALID), (0, 16, ISO_OK), (-1, 16, ISO_ERR_INVALID)):
        assert _raw("iso_upsample_candidates", p(pts), p(knn), rows, K, p(sp), p(cand), L.stream()) == want
        assert _raw("iso_ear_candidates", p(pts), p(nrm), p(knn), p(knn_n), rows, K, 1.0, p(sp), p(cand), L.stream()) == want
    torch.cuda.synchronize()
    assert bool((sp == D.SENTINEL).all()) and bool((cand == D.SENTINEL).all())


# ----------------------------------------------------------------------------------------------- repulse
@pytest.mark.parametrize("P,n,first,K,inv_sigma", D.REPULSE_CASES)
def test_repulse(dev, P, n, first, K, inv_sigma):
    """through UniformProjection.repulsion_step: idx is the [..., 1:] view of the (P, K + 1) list (row stride K + 1),
    with scattered -1, rows of all -1, un-normalised normals and rows of zero normals"""
    from iso_points_amd.levelset_sampling import UniformProjection
    pts, nrm, idx, inv = D.repulse_inputs(P, K)
    if inv_sigma is not None:
        inv = torch.tensor([inv_sigma], dtype=torch.float32)
    ref = D.repulse(pts, nrm, idx[first:first + n, 1:], float(inv), first)
    wide = idx.to(dev)[None, first:first + n]
    view = wide[..., 1:]
    assert view.stride(-2) == K + 1
    proj = UniformProjection(knn_k=max(K, 1))
    out = proj.repulsion_step(pts.to(dev)[None], nrm.to(dev)[None], view, inv.to(dev), first_point=first)
    assert out.shape == (1, n, 3)
    still = D.check_repulse(pts, ref, out[0], first)
    if inv_sigma is not None or K == 0 or n == 1:
        assert still == n
    if K > 0:                                                         # the same list packed (row stride K): same bits
        out2 = proj.repulsion_step(pts.to(dev)[None], nrm.to(dev)[None], view.contiguous(), inv.to(dev), first_point=first)
        assert torch.equal(out, out2)


def test_repulse_direct_and_refusals(dev):
    """the C entry itself: K == 0 with a null idx moves nothing; in-place and idx_row_stride < K are refused unwritten"""
    L = _lib()
    pts, nrm, idx, inv = D.repulse_inputs(1000, 8)
    p, q, i8, s = pts.to(dev), nrm.to(dev), idx[:, 1:].contiguous().to(dev), inv.to(dev)
    out = torch.full((1000, 3), D.SENTINEL, device=dev)
    ptr = L.ptr
    assert _raw("iso_repulse", ptr(p), ptr(q), None, 0, ptr(out), 1000, 0, 0, ptr(s), L.stream()) == ISO_OK
    assert torch.equal(out, p)
    out.fill_(D.SENTINEL)
    keep = p.clone()
    assert _raw("iso_repulse", ptr(p), ptr(q), ptr(i8), 8, ptr(p), 1000, 0, 8, ptr(s), L.stream()) == ISO_ERR_INVALID
    assert _raw("iso_repulse", ptr(p), ptr(q), ptr(i8), 7, ptr(out), 1000, 0, 8, ptr(s), L.stream()) == ISO_ERR_INVALID
    assert _raw("iso_repulse", ptr(p), ptr(q), None, 8, ptr(out), 1000, 0, 8, ptr(s), L.stream()) == ISO_ERR_INVALID
    assert _raw("iso_repulse", ptr(p), ptr(q), ptr(i8), 8, ptr(out), 1000, -1, 8, ptr(s), L.stream()) == ISO_ERR_INVALID
    assert _raw("iso_repulse", ptr(p), ptr(q), ptr(i8), 8, ptr(out), 0, 0, 8, ptr(s), L.stream()) == ISO_OK
    torch.cuda.synchronize()
    assert bool((out == D.SENTINEL).all()) and torch.equal(p, keep)
    L.call("iso_repulse", ptr(p), ptr(q), ptr(i8), 8, ptr(out), 1000, 0, 8, ptr(s), L.stream())
    D.check_repulse(pts, D.repulse(pts, nrm, idx[:, 1:], float(inv)), out)


# ----------------------------------------------------------------------------------------------- insert
def _run_fathers(dev, pts, lens, refs, n_refs, params):
    L = _lib()
    B, P = pts.shape[:2]
    a = pts.to(dev).contiguous()
    ln = None if lens is None else lens.to(dev)
    r, nr, pr = refs.to(dev).contiguous(), torch.tensor([n_refs], dtype=torch.int32, device=dev), params.to(dev)
    father = torch.full((B, P), 7, dtype=torch.uint8, device=dev)
    L.call("iso_insert_fathers", L.ptr(a), L.ptr(ln), B, P, L.ptr(r), L.ptr(nr), L.ptr(pr), L.ptr(father), L.stream())
    return father


@pytest.mark.parametrize("P,lens,n_refs", D.FATHERS_CASES)
def test_insert_fathers(dev, P, lens, n_refs):
    pts, ln, refs, nr, params = D.fathers_inputs(P, lens, n_refs)
    mask, _, fenced = D.fathers(pts, ln, refs, nr, params)
    share = D.check_fathers(mask, fenced, _run_fathers(dev, pts, ln, refs, nr, params))
    print("fenced share %.4f %%" % (100 * share))
    assert share <= 0.01, "fenced share %.4f %%" % (100 * share)


def test_insert_fathers_dyadic(dev):
    """on a reference point, exactly at each limit, one ulp inside and outside: the three strict inequalities, no fence"""
    for pts, refs, nr, params in D.fathers_dyadic():
        mask, _, fenced = D.fathers(pts, None, refs, nr, params)
        assert D.check_fathers(mask, fenced, _run_fathers(dev, pts, None, refs, nr, params), max_fenced=0) == 0


@pytest.mark.parametrize("P,lens,K", D.CHILDREN_CASES)
def test_insert_children(dev, P, lens, K):
    """an index list of width 8, and of width 16 (the LAST eight columns are taken), -1 neighbours, gaps between the
    clouds' rows: the rows no father owns keep the sentinel"""
    L = _lib()
    pts, knn, father, rank, first, n_rows = D.children_inputs(P, lens, K)
    ref = D.children(pts, knn, father, first, 8, n_rows)
    a = [t.to(dev).contiguous() for t in (pts, knn, father, rank, first)]
    out = torch.full((n_rows, 3), D.SENTINEL, device=dev)
    L.call("iso_insert_children", L.ptr(a[0]), L.ptr(a[1]), len(lens), P, K, 8, L.ptr(a[2]), L.ptr(a[3]), L.ptr(a[4]),
           L.ptr(out), L.stream())
    D.check_children(ref, out)


def test_insert_children_refusals(dev):
    L = _lib()
    pts, knn, father, rank, first, n_rows = D.children_inputs(255, [255], 8)
    a = [t.to(dev).contiguous() for t in (pts, knn, father, rank, first)]
    out = torch.full((n_rows, 3), D.SENTINEL, device=dev)
    p = [L.ptr(t) for t in a]
    assert _raw("iso_insert_children", p[0], p[1], 1, 255, 7, 8, p[2], p[3], p[4], L.ptr(out), L.stream()) == ISO_ERR_INVALID
    assert _raw("iso_insert_children", p[0], p[1], 1, 255, 8, 0, p[2], p[3], p[4], L.ptr(out), L.stream()) == ISO_ERR_INVALID
    assert _raw("iso_insert_children", p[0], p[1], 0, 255, 8, 8, p[2], p[3], p[4], L.ptr(out), L.stream()) == ISO_OK
    torch.cuda.synchronize()
    assert bool((out == D.SENTINEL).all())


class _Ref(object):
    def __init__(self, points, metrics, dev):
        self.p, self.f, self.dev = points.to(dev), metrics.to(dev), dev

    def points_packed(self): return self.p
    def features_packed(self): return self.f
    def num_points_per_cloud(self): return torch.tensor([self.p.shape[0]], device=self.dev)
    def __len__(self): return 1


def test_insert_end_to_end_ragged_batch(dev):
    """UniformProjection.insert on a batch of three clouds of 1000, 700 and 0 points against the float64 oracle: the
    selected reference points, the spacing and the radius (through the father sets they decide), the children, the sizes"""
    O = _O()
    from iso_points_amd.levelset_sampling import UniformProjection, with_host_lengths
    ref_p, ref_m, points, lens = D.insert_inputs()
    want = D.insert(ref_p, ref_m, points, lens, O.frnn_grid_points)
    assert float(want["fenced"].float().mean()) == 0
    proj = UniformProjection(knn_k=8)
    num = with_host_lengths(lens.to(dev), lens.tolist())
    grown, n_after, child, cpb = proj.insert(_Ref(ref_p, ref_m, dev), points.to(dev), num)
    assert cpb.tolist() == want["sizes"] and want["sizes"][2] == 0 and min(want["sizes"][:2]) > 0
    assert n_after.tolist() == [int(l) + s for l, s in zip(lens.tolist(), want["sizes"])]
    assert child.shape == (3, max(want["sizes"]), 3) and grown.shape == (3, 1000 + max(want["sizes"]), 3)
    assert torch.equal(grown[:, :1000].cpu(), points) and torch.equal(grown[:, 1000:], child)
    for b in range(3):
        s = want["sizes"][b]
        if s:
            assert rel_err(child[b, :s], want["children"][b]) < D.CHILD_TOL
        assert bool((child[b, s:] == 0).all())
    # a wider current_knn_result: the last eight of its columns mother the children
    _, idx, _, _ = O.frnn_grid_points(points, points, lens, lens, K=9, r=want["radius"])
    wide = torch.cat([torch.full((3, 1000, 8), -1, dtype=torch.int64), idx[..., 1:]], dim=-1)

    class KnnResult(object):
        pass
    kr = KnnResult()
    kr.idx = wide.to(dev)
    _, _, child16, cpb16 = proj.insert(_Ref(ref_p, ref_m, dev), points.to(dev), num, current_knn_result=kr)
    assert cpb16.tolist() == want["sizes"]
    for b in range(2):
        assert rel_err(child16[b, :want["sizes"][b]], want["children"][b]) < D.CHILD_TOL


# ----------------------------------------------------------------------------------------------- host logic around them
def test_upsample_ragged_batch_with_a_full_cloud(dev):
    """point_processing.upsample on a batch of two where one cloud is already full: the reference's `[-0:]` quirk
    (the full cloud still gets a round's rows in front) as oracle.upsample keeps it"""
    O = _O()
    from iso_points_amd.point_processing import upsample
    g = torch.Generator().manual_seed(12)
    pts = torch.rand(2, 300, 3, generator=g)
    lens = torch.tensor([300, 211])
    pts[1, 211:] = 0
    want = torch.tensor([330, 211])
    ref, n_ref = O.upsample(pts, want, num_points=lens.clone(), neighborhood_size=12)
    up, n = upsample(pts.to(dev), want.to(dev), num_points=lens.to(dev), neighborhood_size=12)
    assert torch.equal(n.cpu(), n_ref) and n_ref.tolist() == [330, 211]
    assert not torch.equal(ref[1, :211], pts[1, :211])                  # the quirk: the full cloud's rows were shifted
    assert up.shape == ref.shape == (2, 330, 3) and rel_err(up, ref) < 1e-5


def test_upsample_fewer_than_eight_points(dev):
    """P < 8: max_P == 0, no row can be added and the loop must end with the cloud as it came"""
    from iso_points_amd.point_processing import upsample
    pts = torch.rand(1, 7, 3, generator=torch.Generator().manual_seed(13))
    up, n = upsample(pts.to(dev), 12, neighborhood_size=4)
    assert n.tolist() == [7] and torch.equal(up.cpu(), pts)


def test_wlop_ragged_batch(dev):
    """wlop(ratio=0.25, perturb=False) on a ragged batch of two against oracle.wlop_iterations cloud by cloud"""
    O = _O()
    from iso_points_amd.point_processing import wlop
    from iso_points_amd.levelset_sampling import with_host_lengths
    lens = [2000, 1203]
    P = torch.cat([sphere_cloud(2000, seed=35, jitter=0.02), sphere_cloud(2000, seed=36, jitter=0.02)], dim=0)
    P[1, 1203:] = 0
    X, nX = wlop(P.to(dev), with_host_lengths(torch.tensor(lens, device=dev), lens), ratio=0.25, perturb=False)
    assert nX.tolist() == [500, 301]
    for b in range(2):
        cloud, k = P[b:b + 1, :lens[b]], int(nX[b])
        sel = O.farthest_point_sampling(cloud[0], k, start=0)
        ref = O.wlop_iterations(cloud, torch.tensor([lens[b]]), cloud[:, sel], torch.tensor([k]))
        assert rel_err(X[b:b + 1, :k], ref) < 1e-5
