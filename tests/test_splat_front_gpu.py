"""Stage 1 of the splat pipeline (csrc/splat.hip) on the GPU against the plain references of splat_front_oracle.py:
the renderable mask and its thresholds, the packed layout at chunk and view edges, both entries of the front end, the
feature paths, the row capacity, the set-up's accuracy against float64, the gradient to the world points and the
isotropic bandwidth.  Integer outputs and copies are compared exactly, every packed row bit for bit with k_splat_setup
on the compacted inputs (both call splat_setup_point), arithmetic against float64 under the project's float32 rule
e_hip <= 1.5 e_f32 + 2e-7 with the float32 restatement of the kernel's own statements as e_f32."""
import math

import pytest
import torch

import splat_front_oracle as FO

pytestmark = pytest.mark.gpu

ROW_KEYS = ("ndc", "ellipse_params", "radii", "scaler", "cutoff_threshold")
GUARD, GUARD_I, GUARD_B = 7.0, -7, 9


def _L():
    from iso_points_amd import _lib
    return _lib


def _alloc(rows, C, dev):
    """Output arrays of `rows` rows, pre-filled with guard values."""
    f = lambda *s: torch.full(s, GUARD, dtype=torch.float32, device=dev)                   # noqa: E731
    return {"ndc": f(rows, 3), "ellipse_params": f(rows, 3), "cutoff_threshold": f(rows), "radii": f(rows, 2),
            "scaler": f(rows), "features": f(rows, C) if C else None,
            "src": torch.full((rows,), GUARD_I, dtype=torch.int32, device=dev),
            "visible": torch.full((rows,), GUARD_B, dtype=torch.uint8, device=dev)}


def _dev(dev, *ts):
    return [None if t is None else t.to(dev).contiguous() for t in ts]


def _front(dev, pts, nrm, views, projs, mask, h, S, feat=None, from_normals=False, rows=None, sigma=1.0, cutoff=1.0):
    """iso_splat_front (count, scan, compaction + set-up) on device tensors.  -> outputs, and the scanned chunk table."""
    L = _L()
    p = L.ptr
    P, N = pts.shape[0], views.shape[0]
    C = 3 if from_normals else (feat.shape[1] if feat is not None else 0)
    o = _alloc(max(N * P, 1) if rows is None else rows, C, dev)
    o["first_idx"] = torch.empty((N,), dtype=torch.int64, device=dev)
    o["num_points"] = torch.empty((N,), dtype=torch.int64, device=dev)
    o["view_total"] = torch.full((8,), GUARD_I, dtype=torch.int32, device=dev)
    ws = torch.zeros((L.load().iso_splat_front_workspace_bytes(P),), dtype=torch.uint8, device=dev)
    L.call("iso_splat_front", p(pts), p(nrm), p(feat) if (feat is not None and not from_normals) else None, C,
           int(from_normals), p(mask), p(h), P, p(views), p(projs), N, S, float(sigma), float(cutoff), p(ws), ws.numel(),
           p(o["first_idx"]), p(o["num_points"]), p(o["view_total"]), p(o["ndc"]), p(o["ellipse_params"]),
           p(o["cutoff_threshold"]), p(o["radii"]), p(o["scaler"]), p(o["features"]), p(o["src"]), L.stream())
    return o, ws


def _front_rows(dev, pts, nrm, views, projs, mask, h, S, ws, first, rows, cap, feat=None, from_normals=False,
                sigma=1.0, cutoff=1.0):
    """iso_splat_front_rows on a scanned chunk table: arrays of `rows` rows, of which the call may write `cap`."""
    L = _L()
    p = L.ptr
    P, N = pts.shape[0], views.shape[0]
    C = 3 if from_normals else (feat.shape[1] if feat is not None else 0)
    o = _alloc(rows, C, dev)
    o["row_overflow"] = torch.zeros((1,), dtype=torch.int32, device=dev)
    L.call("iso_splat_front_rows", p(pts), p(nrm), p(feat) if (feat is not None and not from_normals) else None, C,
           int(from_normals), p(mask), p(h), P, p(views), p(projs), N, S, float(sigma), float(cutoff), p(ws), ws.numel(),
           p(first), p(o["ndc"]), p(o["ellipse_params"]), p(o["cutoff_threshold"]), p(o["radii"]), p(o["scaler"]),
           p(o["features"]), p(o["src"]), p(o["visible"]), int(cap), p(o["row_overflow"]), L.stream())
    return o


def _setup(dev, pts_c, nrm_c, h_c, first, num, views, projs, S, sigma=1.0, cutoff=1.0):
    """iso_splat_setup (k_splat_setup) on already compacted rows."""
    L = _L()
    p = L.ptr
    T = pts_c.shape[0]
    o = _alloc(max(T, 1), 0, dev)
    if T:
        L.call("iso_splat_setup", p(pts_c), p(nrm_c), p(h_c), p(first), p(num), p(views), p(projs), views.shape[0],
               int(num.max().item()), S, float(sigma), float(cutoff), p(o["ndc"]), p(o["ellipse_params"]),
               p(o["cutoff_threshold"]), p(o["radii"]), p(o["scaler"]), L.stream())
    return o


def _compacted(pts, nrm, h, first, num, src):
    """The compacted inputs of the packed layout (CPU tensors): points, normals, h of every row."""
    s = src.long()
    view_of = torch.repeat_interleave(torch.arange(num.numel()), num)
    return pts[s].contiguous(), nrm[s].contiguous(), h[view_of, s].contiguous()


def _assert_rows_equal_setup(dev, got, pts, nrm, h, views, projs, S, first, num, src, sel=None, what=""):
    """Every packed row (or the rows `sel`) equals k_splat_setup on the compacted inputs, bit for bit."""
    pc, nc, hc = _compacted(pts, nrm, h, first, num, src)
    T = int(num.sum())
    ref = _setup(dev, *_dev(dev, pc, nc, hc, first, num), views, projs, S)
    rows = slice(0, T) if sel is None else sel
    for k in ROW_KEYS:
        a, b = got[k][:T][rows], ref[k][:T][rows]
        assert torch.equal(a, b), "%s %s: %d rows differ from k_splat_setup" % (
            what, k, int((a != b).reshape(a.shape[0], -1).any(-1).sum()))


def _cameras(n_views):
    from oracle import splat_oracle as SO
    views = torch.stack([SO.look_at_view(3.0 + 0.25 * i, 20.0 - 9.0 * i, 47.0 * i) for i in range(n_views)])
    projs = torch.stack([v @ SO.perspective(30.0) for v in views])
    return views.contiguous(), projs.contiguous()


def _cloud(P, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    nrm = torch.nn.functional.normalize(pts + 0.1 * torch.randn(P, 3, generator=g), dim=-1)
    return pts.contiguous(), nrm.contiguous(), g


# ----------------------------------------------------------------------------- a. packing is exact
LANE_SPOTS = [(lane, k) for k in range(4) for lane in (0, 63, 64, 255)]


def _hand_masks(P, N, g):
    all_v = (1 << N) - 1
    masks = {"all": torch.full((P,), all_v, dtype=torch.int64)}
    empty_view = N // 2
    masks["empty_view"] = torch.full((P,), all_v & ~(1 << empty_view), dtype=torch.int64)
    one = torch.zeros(P, dtype=torch.int64)
    for c in range((P + FO.CHUNK - 1) // FO.CHUNK):
        for v in range(N):
            lane, k = LANE_SPOTS[(c * N + v) % 16]
            i = c * FO.CHUNK + lane * 4 + k
            if i < P:
                one[i] |= 1 << v
    masks["one_per_chunk"] = one
    for name, dens in (("half", 0.5), ("sparse", 0.01)):
        fl = torch.rand(N, P, generator=g) < dens
        masks[name] = FO.mask_bits(fl).long()
    return {k: m.to(torch.int32) for k, m in masks.items()}


@pytest.mark.parametrize("n_views", [1, 2, 5, 8])
@pytest.mark.parametrize("P", [1, 3, 255, 256, 1023, 1024, 1025, 2049, 4100])
def test_packing_is_exact(dev, P, n_views):
    """Hand-made masks through iso_splat_front: first_idx, num_points, view_total and src equal the plain layout; every
    row equals k_splat_setup on the compacted inputs bit for bit."""
    pts, nrm, g = _cloud(P, 100 * P + n_views)
    views, projs = _cameras(n_views)
    h = torch.rand(n_views, P, generator=g) * 0.01
    S = 64
    dp, dn, dv, dm, dh = _dev(dev, pts, nrm, views, projs, h)
    for name, mask in _hand_masks(P, n_views, g).items():
        first, num, src = FO.pack_ref(mask, n_views)
        T = int(num.sum())
        got, _ = _front(dev, dp, dn, dv, dm, mask.to(dev), dh, S)
        assert torch.equal(got["first_idx"].cpu(), first) and torch.equal(got["num_points"].cpu(), num), name
        assert torch.equal(got["view_total"].cpu(), FO.view_total_ref(num)), name
        assert torch.equal(got["src"][:T].cpu(), src), name
        assert (got["src"][T:] == GUARD_I).all() and (got["scaler"][T:] == GUARD).all(), name   # nothing past the rows
        _assert_rows_equal_setup(dev, got, pts, nrm, h, dv, dm, S, first, num, src, what=name)
        if name == "empty_view" and n_views > 1:
            assert num[n_views // 2] == 0
        if name == "all":
            assert T == n_views * P


def test_packing_past_one_lap_of_the_chunk_scan(dev):
    """P = 1 048 577: 1025 chunks, so the one-workgroup scan of the chunk counts takes a second lap and the last chunk
    holds one point.  Integer outputs exactly; the rows of the last two chunks bit for bit."""
    P, N, S = 1048577, 2, 64
    pts, nrm, g = _cloud(P, 77)
    views, projs = _cameras(N)
    fl = torch.rand(N, P, generator=g) < 0.5
    fl[:, P - 1] = True
    fl[0, (P - 1) - FO.CHUNK:(P - 1)] = True                # chunk 1023 full in view 0
    fl[1, (P - 1) - FO.CHUNK:(P - 1)] = False               # ... and without a row in view 1
    mask = FO.mask_bits(fl)
    h = torch.rand(N, P, generator=g) * 0.01
    first, num, src = FO.pack_ref(fl, N)
    T = int(num.sum())
    dp, dn, dv, dm, dh = _dev(dev, pts, nrm, views, projs, h)
    got, _ = _front(dev, dp, dn, dv, dm, mask.to(dev), dh, S, rows=T + 8)
    assert torch.equal(got["first_idx"].cpu(), first) and torch.equal(got["num_points"].cpu(), num)
    assert torch.equal(got["view_total"].cpu(), FO.view_total_ref(num))
    assert torch.equal(got["src"][:T].cpu(), src) and (got["src"][T:] == GUARD_I).all()
    tail = torch.nonzero(src.long() >= (P - 1) - FO.CHUNK).flatten()
    assert tail.numel() == FO.CHUNK + 2
    _assert_rows_equal_setup(dev, got, pts, nrm, h, dv, dm, S, first, num, src, sel=tail.to(dev))


# ----------------------------------------------------------------------------- b. both entries, thresholds
def _axis_views(N):
    """Axis-aligned rotations (signed permutations of determinant +1) with dyadic translations, and their projections."""
    from oracle import splat_oracle as SO
    rots = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]],
            [[-1, 0, 0], [0, 1, 0], [0, 0, -1]], [[0, 0, -1], [0, 1, 0], [1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
            [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, -1, 0], [0, 0, -1]]]
    shifts = [[0.0, 0.0, 2.0], [0.25, -0.5, 1.75], [0.0, 0.125, 2.5], [-0.75, 0.0, 2.25], [0.5, 0.5, 1.5],
              [0.0, 0.0, 3.0], [0.125, 0.25, 2.0], [-0.25, 0.375, 1.875]]
    views = []
    for r, t in zip(rots[:N], shifts[:N]):
        V = torch.eye(4)
        V[:3, :3] = torch.tensor(r, dtype=torch.float32)
        V[3, :3] = torch.tensor(t)
        views.append(V)
    views = torch.stack(views)
    return views.contiguous(), torch.stack([v @ SO.perspective(30.0) for v in views]).contiguous()


def _lattice_cloud(P, seed):
    """Points on the lattice of 1/8 in [-1.5, 1.5]^3 and normals from {-1, -0.5, 0, 0.5, 1}^3: z_view and the view-space
    normal are exact in float32, and many of them sit exactly on znear, zfar and 0."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.randint(-12, 13, (P, 3), generator=g).float() / 8.0
    nrm = torch.randint(-2, 3, (P, 3), generator=g).float() / 2.0
    return pts.contiguous(), nrm.contiguous(), g


@pytest.mark.parametrize("backface", [False, True])
@pytest.mark.parametrize("P,N", [(1, 1), (1025, 5), (2049, 2), (4100, 8)])
def test_mask_kernels_and_both_entries(dev, P, N, backface):
    """z slabs (culling off) and flipped normals (culling on) on exactly representable geometry: iso_splat_view_flags,
    iso_splat_view_mask, iso_splat_view_mask_scan and iso_compact_rows equal the plain references, points exactly on
    znear / zfar are in and normals with zero view-space z are out; iso_splat_front and iso_splat_view_mask_scan +
    iso_splat_front_rows give the same rows, all of them, equal to the plain layout and to k_splat_setup."""
    L = _L()
    p = L.ptr
    znear, zfar, S = 1.0, 2.5, 48
    pts, nrm, g = _lattice_cloud(P, 31 * P + N)
    views, projs = _axis_views(N)
    if P > 1:                                               # rows on each threshold, by construction, in view 0
        pts[0], nrm[0] = torch.tensor([0.0, 0.0, -1.0]), torch.tensor([0.0, 0.0, -1.0])      # zv == znear: in
        pts[1], nrm[1] = torch.tensor([0.0, 0.0, 0.5]), torch.tensor([0.0, 0.0, -1.0])       # zv == zfar: in
        pts[2], nrm[2] = torch.tensor([0.0, 0.0, 0.0]), torch.tensor([1.0, -1.0, 0.0])       # nzv == 0: out when culling
    else:
        pts[0], nrm[0] = torch.tensor([0.0, 0.0, -1.0]), torch.tensor([0.0, 0.0, -1.0])
    fl = FO.flags_ref(pts, nrm, views, znear, zfar, backface)
    assert torch.equal(fl, FO.mask64(pts, nrm, views, znear, zfar, backface))                 # exact geometry
    if P > 1:
        assert fl[0, 0] and fl[0, 1] and bool(fl[0, 2]) == (not backface)
        zv = pts.double() @ views[:, :3, 2].double().T + views[:, 3, 2].double()
        assert ((zv == znear).sum() > 3) and ((zv == zfar).sum() > 3)
        assert ((nrm.double() @ views[:, :3, 2].double().T) == 0).sum() > 3
    bits = FO.mask_bits(fl)
    first, num, src = FO.pack_ref(fl, N)
    T = int(num.sum())
    dp, dn, dv, dm = _dev(dev, pts, nrm, views, projs)
    # the three mask kernels
    flags = torch.full((N * P + 1,), GUARD_I, dtype=torch.int32, device=dev)
    L.call("iso_splat_view_flags", p(dp), p(dn), p(dv), p(flags), P, N, znear, zfar, int(backface), L.stream())
    assert torch.equal(flags[:N * P].view(N, P).cpu(), fl.int()) and flags[N * P] == GUARD_I
    m0 = torch.full((P + 1,), GUARD_I, dtype=torch.int32, device=dev)
    cnt = torch.empty((8,), dtype=torch.int32, device=dev)
    L.call("iso_splat_view_mask", p(dp), p(dn), p(dv), N, P, znear, zfar, int(backface), p(m0), p(cnt), L.stream())
    assert torch.equal(m0[:P].cpu(), bits) and m0[P] == GUARD_I and torch.equal(cnt.cpu(), FO.view_total_ref(num))
    m1 = torch.full((P + 1,), GUARD_I, dtype=torch.int32, device=dev)
    ws = torch.zeros((L.load().iso_splat_front_workspace_bytes(P),), dtype=torch.uint8, device=dev)
    f1 = torch.empty((N,), dtype=torch.int64, device=dev)
    n1 = torch.empty((N,), dtype=torch.int64, device=dev)
    t1 = torch.empty((8,), dtype=torch.int32, device=dev)
    L.call("iso_splat_view_mask_scan", p(dp), p(dn), p(dv), N, P, znear, zfar, int(backface), p(m1), p(ws), ws.numel(),
           p(f1), p(n1), p(t1), L.stream())
    assert torch.equal(m1[:P].cpu(), bits) and m1[P] == GUARD_I
    assert torch.equal(f1.cpu(), first) and torch.equal(n1.cpu(), num) and torch.equal(t1.cpu(), FO.view_total_ref(num))
    # compaction of U-wide rows by the flags and their exclusive scan
    off = (torch.cumsum(flags[:N * P], 0) - flags[:N * P]).to(torch.int32)
    for U in (1, 3, 5):
        x = torch.randn(P, U, generator=g)
        out = torch.full((T + 1, U), GUARD, device=dev)
        L.call("iso_compact_rows", p(x.to(dev)), p(flags), p(off), p(out), P, N * P, U, L.stream())
        assert torch.equal(out[:T].cpu(), x[src.long()]) and (out[T] == GUARD).all(), U
    # both entries of the front end
    h = torch.rand(N, P, generator=g) * 0.01
    dh = h.to(dev)
    feat = torch.randn(P, 5, generator=g)
    a, _ = _front(dev, dp, dn, dv, dm, m0[:P].contiguous(), dh, S, feat=feat.to(dev), rows=T + 4)
    b = _front_rows(dev, dp, dn, dv, dm, m1[:P].contiguous(), dh, S, ws, f1, T + 4, 0, feat=feat.to(dev))
    assert torch.equal(a["first_idx"], f1) and torch.equal(a["num_points"], n1) and torch.equal(a["view_total"], t1)
    assert int(b["row_overflow"].item()) == 0
    for k in ROW_KEYS + ("features", "src"):
        assert torch.equal(a[k], b[k]), k                   # every row, and the guard rows past them
    assert torch.equal(a["src"][:T].cpu(), src) and (a["src"][T:] == GUARD_I).all()
    assert torch.equal(a["features"][:T].cpu(), feat[src.long()])
    assert (b["visible"][:T] == 0).all() and (b["visible"][T:] == GUARD_B).all()
    _assert_rows_equal_setup(dev, a, pts, nrm, h, dv, dm, S, first, num, src)


# ----------------------------------------------------------------------------- c. features
@pytest.mark.parametrize("C", [0, 1, 3, 4, 8, "normals"])
def test_features(dev, C):
    """C of 1 to 3 is staged in LDS, 4 to 8 written directly, `features_from_normals` computed in the kernel:
    features[row] == input[src[row]] exactly; from normals, 0.5 (n / max(|n|, 1e-12) + 1) of float64 within 2 ulp of
    the output range's top binade (2^-24: the statement's float32 rounding is bounded by 1.75 of them -- sum of
    squares 2, root 0.5 + 1, quotient 1, the + 1 one, halved)."""
    P, N, S = 2300, 3, 64
    pts, nrm, g = _cloud(P, 5)
    nrm[::3] *= 0.1
    nrm[1::3] *= 10.0
    nrm[[0, 5, 1023, 1024, P - 1]] = 0.0                     # the 1e-12 clamp
    nrm[7] = torch.tensor([3e-13, 0.0, -4e-13])             # shorter than the clamp
    nrm[8] = torch.tensor([0.0, 0.0, -2.5])
    views, projs = _cameras(N)
    fl = torch.rand(N, P, generator=g) < 0.5
    fl[:, [0, 5, 7, 8, 1023, 1024, P - 1]] = True
    mask = FO.mask_bits(fl)
    first, num, src = FO.pack_ref(fl, N)
    T = int(num.sum())
    h = torch.rand(N, P, generator=g) * 0.01
    from_normals = C == "normals"
    feat = torch.randn(P, C, generator=g) if (not from_normals and C) else None
    dp, dn, dv, dm, dh, df = _dev(dev, pts, nrm, views, projs, h, feat)
    got, ws = _front(dev, dp, dn, dv, dm, mask.to(dev), dh, S, feat=df, from_normals=from_normals, rows=T + 4)
    rows = _front_rows(dev, dp, dn, dv, dm, mask.to(dev), dh, S, ws, got["first_idx"], T + 4, 0, feat=df,
                       from_normals=from_normals)
    for o in (got, rows):
        assert torch.equal(o["src"][:T].cpu(), src)
        for k in ("ndc", "ellipse_params", "radii", "scaler"):
            assert torch.isfinite(o[k][:T]).all(), k          # zero normals included
        if C == 0:
            assert o["features"] is None
        elif not from_normals:
            assert torch.equal(o["features"][:T].cpu(), feat[src.long()])
            assert (o["features"][T:] == GUARD).all()
        else:
            n64 = nrm.double()[src.long()]
            want = 0.5 * (n64 / n64.norm(dim=-1, keepdim=True).clamp(min=float(torch.tensor(1e-12, dtype=torch.float32))) + 1.0)
            err = (o["features"][:T].cpu().double() - want).abs().max().item()
            print("features from normals: max error %.3g = %.2f ulp (2^-24)" % (err, err * 2 ** 24))
            assert err <= 2.0 * 2.0 ** -24
            zero = (n64 == 0).all(-1)
            assert zero.sum() >= 5 * N and (o["features"][:T].cpu()[zero] == 0.5).all()
            assert (o["features"][T:] == GUARD).all()
    _assert_rows_equal_setup(dev, got, pts, nrm, h, dv, dm, S, first, num, src)


# ----------------------------------------------------------------------------- d. capacity
@pytest.mark.parametrize("which", ["last", "middle"])
@pytest.mark.parametrize("C", [3, 5])
def test_row_capacity(dev, C, which):
    """iso_splat_front_rows with a row capacity at, inside and before a chunk's rows of a view: the flag is raised iff
    rows were dropped, nothing at or past `cap` is written in any array, and ALL rows below `cap` -- the cut view
    included -- equal the unbounded call, features, src and the cleared `visible` flags too."""
    from iso_points_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    P, N, S = 4100, 3, 64
    pts, nrm, g = _cloud(P, 9)
    views, projs = _cameras(N)
    fl = torch.rand(N, P, generator=g) < 0.6
    fl[N - 1, P - 3:] = True                                # the last chunk (4 points) has three rows in the last view
    mask = FO.mask_bits(fl)
    first, num, src = FO.pack_ref(fl, N)
    T = int(num.sum())
    h = torch.rand(N, P, generator=g) * 0.01
    feat = torch.randn(P, C, generator=g)
    dp, dn, dv, dm, dh, df = _dev(dev, pts, nrm, views, projs, h, feat)
    full, ws = _front(dev, dp, dn, dv, dm, mask.to(dev), dh, S, feat=df, rows=T + 64)
    assert torch.equal(full["src"][:T].cpu(), src)
    # a chunk's first row and row count in one view: the last chunk of the last view (p0 + cnt == T), or a middle one
    v, c = (N - 1, (P - 1) // FO.CHUNK) if which == "last" else (1, 2)
    in_chunk = fl[v, c * FO.CHUNK:(c + 1) * FO.CHUNK]
    p0, cnt = int(first[v]) + int(fl[v, :c * FO.CHUNK].sum()), int(in_chunk.sum())
    assert cnt > 1 and (p0 + cnt == T) == (which == "last")
    for cap in (T, p0 + cnt, p0 + cnt - 1, p0 + 1, p0, 1):
        o = _front_rows(dev, dp, dn, dv, dm, mask.to(dev), dh, S, ws, full["first_idx"], T + 64, cap, feat=df)
        n = min(cap, T)
        assert int(o["row_overflow"].item()) == int(cap < T), cap
        for k in ROW_KEYS + ("features", "src"):
            assert torch.equal(o[k][:n], full[k][:n]), (cap, k)
            assert (o[k][n:] == (GUARD_I if k == "src" else GUARD)).all(), (cap, k)
        assert (o["visible"][:n] == 0).all() and (o["visible"][n:] == GUARD_B).all(), cap
    # the same through SurfaceSplatting.front_setup: its (12, cap) buffer with a guard region behind it
    if C == 3:
        ss = SurfaceSplatting(raster_settings=PointsRasterizationSettings(image_size=S))
        scanned = (ws, full["first_idx"], full["num_points"], full["view_total"])
        try:
            for cap in (T, p0 + cnt, p0 + cnt - 1, p0 + 1, p0, 1):
                ss._row_overflow = None                      # sticky on the object: a fresh flag for every capacity
                guard = torch.full((12 * cap + 4096,), GUARD, device=dev)
                o = ss.front_setup(dp, dn, dv, dm, mask.to(dev), dh, features=df, scanned=scanned, out=guard, capacity=cap)
                assert int(o["row_overflow"].item()) == int(cap < T)
                assert (guard[12 * cap:] == GUARD).all()
                for k in ("ndc", "ellipse_params", "radii", "scaler", "features", "src", "cutoff_threshold"):
                    assert torch.equal(o[k][:min(cap, T)], full[k][:min(cap, T)]), (cap, k)
                assert (o["visible"][:min(cap, T)] == 0).all()
        finally:
            ss._row_overflow = None                          # the sticky flag of this object


# ----------------------------------------------------------------------------- e. set-up accuracy against float64
_worst = {}


@pytest.mark.parametrize("normals", FO.NORMALS)
@pytest.mark.parametrize("cam", FO.CAMERAS)
def test_setup_accuracy_against_float64(dev, cam, normals):
    """Per row and output, the error against setup64 at the quantiles 0.5, 0.9, 0.99 and 1: e_hip <= 1.5 e_setup32 +
    2e-7, setup32 being the float32 restatement of the kernel's statements (expansion of det G; radii from g00, g11).
    Measured on an MI355X over all cases: the kernel equals setup32 bit for bit in every row, so the worst
    e_hip / limit is the yardstick's against itself -- ndc 0.29, ellipse 0.66, radii 0.49, scaler 0.67 (front
    end).  With the reference's radii statement sqrt(4c cutoff / (4ac - b^2)) the radii are up to 594 times over the limit
    (3.5e-4 against 3.6e-7 now: perspective, grazing, S = 1040, h = 0.01)."""
    V, M = FO.camera(cam)
    dv, dm = _dev(dev, V[None], M[None])
    misses = []
    for S in FO.SIZES:
        pts, nrm = FO.case_cloud(normals, V, seed=S)
        P = pts.shape[0]
        dp, dn = _dev(dev, pts, nrm)
        mask = torch.ones(P, dtype=torch.int32, device=dev)
        for h in FO.BANDWIDTHS:
            hk = torch.full((P,), h)
            got, _ = _front(dev, dp, dn, dv, dm, mask, hk.to(dev).view(1, P).contiguous(), S)
            assert int(got["num_points"][0]) == P
            got = {k: got[k][:P].cpu() for k in FO.OUTPUTS}
            for k in FO.OUTPUTS:
                assert torch.isfinite(got[k]).all(), (S, h, k)
            truth = FO.setup64(pts, nrm, hk, V, M, S)
            y32 = FO.setup32(pts, nrm, hk, V, M, S)
            e_hip, e_32 = FO.row_errors(got, truth), FO.row_errors(y32, truth)
            for k in FO.OUTPUTS:
                qh, q32 = FO.quantiles(e_hip[k]), FO.quantiles(e_32[k])
                ratio = max(a / (1.5 * b + 2e-7) for a, b in zip(qh, q32))
                same = (got[k] == y32[k]).reshape(P, -1).all(-1).float().mean().item()
                print("%s %s S=%d h=%g %-14s e_hip %s  e_setup32 %s  e_hip/limit %.3f  rows equal to setup32 %.4f"
                      % (cam, normals, S, h, k, " ".join("%.2e" % x for x in qh), " ".join("%.2e" % x for x in q32),
                         ratio, same))
                _worst[k] = max(_worst.get(k, 0.0), ratio)
                if not ratio <= 1.0:
                    misses.append((S, h, k, round(ratio, 3), qh, q32))
    print("worst e_hip / limit so far: %s" % {k: round(v, 3) for k, v in _worst.items()})
    assert not misses, misses


def test_setup_is_finite_for_a_zero_normal_and_zero_bandwidth(dev):
    V, M = FO.camera("perspective")
    pts, nrm = FO.case_cloud("radial", V, seed=2, P=300)
    nrm[::2] = 0.0
    hk = torch.zeros(300)
    hk[::3] = 0.01
    dp, dn, dv, dm = _dev(dev, pts, nrm, V[None], M[None])
    got, _ = _front(dev, dp, dn, dv, dm, torch.ones(300, dtype=torch.int32, device=dev), hk.to(dev).view(1, -1).contiguous(), 64)
    y32 = FO.setup32(pts, nrm, hk, V, M, 64)
    for k in FO.OUTPUTS:
        assert torch.isfinite(got[k][:300]).all(), k
        assert torch.equal(got[k][:300].cpu()[::2], y32[k][::2]), k          # a zero frame: every statement is exact
    assert (got["scaler"][:300][::2] == 0).all()


def test_helper_axis_on_ties(dev):
    """Normals whose two or three smallest components tie ((1, 1, 2), (1, 1, 1), the axes ...): the helper axis is the
    first of the tied ones, x before y before z (vrk_util.kernel_tangent_frame and splat_setup_frame's callers rely on
    it: iso_splat_tangent_frame exports the frame).  Another tied axis gives another, equally valid frame and other
    rounding, so this is checked bit for bit against the float32 restatement, which the kernel reproduces exactly."""
    V, M = FO.camera("off_axis")
    pts, nrm = FO.case_cloud("axis_ties", V, seed=4, P=1200)
    nrm = nrm[::2].contiguous()                               # the un-normalised ones: small integers, ties exact
    pts = pts[::2].contiguous()
    P = pts.shape[0]
    hk = torch.full((P,), 0.003)
    dp, dn, dv, dm = _dev(dev, pts, nrm, V[None], M[None])
    got, _ = _front(dev, dp, dn, dv, dm, torch.ones(P, dtype=torch.int32, device=dev), hk.to(dev).view(1, -1).contiguous(), 64)
    y32 = FO.setup32(pts, nrm, hk, V, M, 64)
    for k in FO.OUTPUTS:
        bad = (got[k][:P].cpu() != y32[k]).reshape(P, -1).any(-1)
        assert not bad.any(), "%s: %d rows differ from the float32 restatement, e.g. normal %s" % (
            k, int(bad.sum()), nrm[bad][0].tolist())
    u, v = torch.empty_like(dn), torch.empty_like(dn)
    L = _L()
    L.call("iso_splat_tangent_frame", L.ptr(dn), P, L.ptr(u), L.ptr(v), L.stream())
    (ux, uy, uz), (vx, vy, vz) = FO._frame(nrm)
    assert torch.equal(u.cpu(), torch.stack([ux, uy, uz], -1)) and torch.equal(v.cpu(), torch.stack([vx, vy, vz], -1))


# ----------------------------------------------------------------------------- f. gradient to the world points
@pytest.mark.parametrize("P", [1, 1025, 5000])
@pytest.mark.parametrize("n_views", [1, 5, 8])
@pytest.mark.parametrize("pattern", ["empty_view", "all_views"])
def test_points_backward(dev, pattern, n_views, P):
    """iso_splat_points_backward on hand-made mask / src / first / num, against float64 autograd under the float32 rule,
    scaled by each point's sum of |terms|; a point no view renders gets exactly 0.  Two mask patterns (one mask cannot
    hold both): `empty_view` -- view n_views // 2 has no row (num == 0; with one view there is no such view), points 0
    and P - 1 own the first and the last row of every other view (the ends of the kernel's binary search);
    `all_views` -- no view is emptied and points 0 and P - 1 carry every bit (0xFF with 8 views), so the kernel's view
    loop accumulates all n_views terms into one point, and they own the first and the last row of every view."""
    L = _L()
    p = L.ptr
    pts, _, g = _cloud(P, 1000 * n_views + P + (7 if pattern == "all_views" else 0))
    views, projs = _cameras(n_views)
    fl = torch.rand(n_views, P, generator=g) < 0.4
    live = list(range(n_views))
    if pattern == "empty_view" and n_views > 1:
        fl[n_views // 2] = False                             # num == 0
        live.remove(n_views // 2)
    fl[live, 0] = True                                       # owns row 0 of every live view
    fl[live, P - 1] = True                                   # owns the last row
    if P > 2:
        fl[:, P // 2] = False                                # rendered nowhere
        fl[live[0], 1] = False                               # row 1 of the first view belongs to a later point
    if pattern == "all_views":
        assert int(FO.mask_bits(fl)[0]) == (1 << n_views) - 1 == int(FO.mask_bits(fl)[P - 1]) and fl.any(1).all()
    elif n_views > 1:
        assert not fl[n_views // 2].any()
    first, num, src = FO.pack_ref(fl, n_views)
    T = int(num.sum())
    gn = torch.randn(T, 3, generator=g)
    mask = FO.mask_bits(fl)
    out = torch.full((P, 3), GUARD, device=dev)
    dp, dv, dm, dmask, dsrc, dfirst, dnum, dgn = _dev(dev, pts, views, projs, mask, src, first, num, gn)
    L.call("iso_splat_points_backward", p(dp), P, p(dv), p(dm), n_views, p(dmask), p(dsrc), p(dfirst), p(dnum), p(dgn),
           p(out), L.stream())
    got = out.cpu()
    truth, scale = FO.points_backward64(pts, views, projs, fl, first, src, gn)
    y32 = FO.points_backward32(pts, views, projs, fl, first, src, gn)
    seen = fl.any(0)
    assert (got[~seen] == 0).all() and (truth[~seen] == 0).all()
    assert seen[0] and seen[P - 1] and torch.isfinite(got).all()
    sc = scale[seen].clamp(min=1e-300)
    e_hip = (got.double() - truth)[seen].abs().amax(-1) / sc
    e_32 = (y32.double() - truth)[seen].abs().amax(-1) / sc
    qh, q32 = FO.quantiles(e_hip), FO.quantiles(e_32)
    ratio = max(a / (1.5 * b + 2e-7) for a, b in zip(qh, q32))
    print("points backward %s N=%d P=%d: e_hip %s  e_f32 %s  e_hip/limit %.3f  equal to the float32 restatement: %s"
          % (pattern, n_views, P, " ".join("%.2e" % x for x in qh), " ".join("%.2e" % x for x in q32), ratio, torch.equal(got, y32)))
    assert ratio <= 1.0, (qh, q32)
    # the end rows by themselves: their error is in the maximum above, but say so
    for i in (0, P - 1):
        assert (got[i].double() - truth[i]).abs().max().item() <= (1.5 * q32[-1] + 2e-7) * max(scale[i].item(), 1e-300)


# ----------------------------------------------------------------------------- g. isotropic bandwidth
def test_vrk_h(dev):
    """iso_splat_vrk_h == clamp(0.5 max of columns 1..6, 5e-5, 0.01) exactly: rows with 6, 3 and no hit (-1 as FRNN
    leaves them), values on and next to both clamps, a cloud of 6 points (every distance taken as 1e-3), and the
    optional per-cloud length that decides that branch."""
    L = _L()
    p = L.ptr
    g = torch.Generator().manual_seed(3)
    lens, pmax = [700, 6, 300, 0], 700
    d = torch.rand(4, pmax, 7, generator=g) * 0.03
    d[:, :, 0] = 0.0
    d[0, 100:200, 4:] = -1.0                                  # 3 hits
    d[0, 200:300, 1:] = -1.0                                  # no hit
    d[0, 300:400] *= 1e-3                                     # below the lower clamp
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    for j, m in enumerate((1e-4, 0.02)):                      # 0.5 m on the clamp, and one float to either side
        for k, val in enumerate((f32(m), torch.nextafter(f32(m), f32(1.0)), torch.nextafter(f32(m), f32(0.0)))):
            d[0, 400 + 3 * j + k, 1:] = -1.0
            d[0, 400 + 3 * j + k, 3] = val
    d[1] = torch.rand(pmax, 7, generator=g)                   # 6 points: never read
    num = torch.tensor(lens)
    first = torch.cumsum(num, 0) - num
    tot = int(num.sum())
    dd, dfirst, dnum = _dev(dev, d, first, num)
    for cloud_num in (None, torch.tensor([700, 9, 5, 0])):
        h = torch.full((tot + 1,), GUARD, device=dev)
        L.call("iso_splat_vrk_h", p(dd), p(dfirst), p(dnum), p(cloud_num.to(dev)) if cloud_num is not None else None, p(h),
               4, pmax, L.stream())
        want = FO.vrk_h_ref(d, num, cloud_num)
        assert torch.equal(h[:tot].cpu(), want) and h[tot] == GUARD
        assert (want == f32(5e-5)).sum() > 200 and (want == f32(0.01)).sum() > 100
        assert (want[700:706] == (f32(0.5) * f32(1e-3)).item()).all() == (cloud_num is None)
    assert math.isclose(float(want[400]), 5e-5, rel_tol=1e-6) and float(want[401]) > float(want[400]) == float(want[402])
