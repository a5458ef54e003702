"""iso_points_amd.point_processing.remove_close and iso_points_amd.ops.sample_points_from_meshes_even on the GPU against the
serial rule of include/isopoints.h section L restated in numpy (tests/disk_oracle.py: brute force, the float32 d2 <= r2).
Every comparison is exact equality of mask, sel and kept, with the oracle run on the bits the GPU was given.

Shapes: clouds of up to 4 000 points.  A cloud of up to 2 048 points gets a grid of at most 16 cells per axis, a larger one
of at most 48, so both appear; the round kernel runs 256 lanes per workgroup (more than one workgroup from 257 points on)
and the compaction works in tiles of 2 048 samples (4 000 points: two tiles, the second partly filled; 2 048: exactly one;
3 000: one and a part)."""
import numpy as np
import pytest
import torch

import disk_oracle as D
from disk_oracle import SAMPLER_CASES, sampler_mesh

pytestmark = pytest.mark.gpu


def run(dev, pts, radius, lengths=None, valid=None):
    """remove_close on numpy inputs: (mask (N,P) bool, sel (N,P) int64, kept (N,) int64) as numpy."""
    from iso_points_amd.point_processing import remove_close
    pts = np.asarray(pts, dtype=np.float32)
    if pts.ndim == 2:
        pts = pts[None]
    if isinstance(radius, (list, tuple, np.ndarray)):
        radius = torch.tensor(np.asarray(radius, dtype=np.float32), device=dev)
    mask, sel, kept = remove_close(torch.from_numpy(pts).to(dev), radius,
                                   None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=dev),
                                   None if valid is None else torch.from_numpy(np.asarray(valid)).to(dev))
    assert mask.dtype == torch.bool and sel.dtype == torch.int64 and kept.dtype == torch.int64
    assert tuple(mask.shape) == pts.shape[:2] and tuple(sel.shape) == pts.shape[:2] and tuple(kept.shape) == pts.shape[:1]
    return mask.cpu().numpy(), sel.cpu().numpy(), kept.cpu().numpy()


def check(got, pts, radius, lengths=None, valid=None):
    """got = run(...) against the oracle, cloud by cloud; returns the oracle's masks."""
    pts = np.asarray(pts, dtype=np.float32)
    if pts.ndim == 2:
        pts = pts[None]
    mask, sel, kept = got
    want = []
    for n in range(len(pts)):
        r = radius[n] if isinstance(radius, (list, tuple, np.ndarray)) else radius
        m, s, k = D.serial(pts[n], r, None if lengths is None else lengths[n], None if valid is None else np.asarray(valid)[n])
        assert (mask[n] == m).all(), (n, np.nonzero(mask[n] != m)[0][:10])
        assert (sel[n] == s).all() and kept[n] == k, (n, kept[n], k)
        want.append(m)
    return want


_CASE1 = {}


def case1(dev):
    """3 000 points on the unit sphere at r = 0.065: the cloud, what the GPU returns and the oracle's mask, computed once."""
    if not _CASE1:
        pts = D.sphere_cloud(3000, 11)
        got = run(dev, pts, 0.065)
        _CASE1.update(pts=pts, got=got, want=check(got, pts, 0.065)[0])
    return _CASE1


def test_basic_sphere(dev):
    c = case1(dev)
    kept = int(c["got"][2][0])
    print("3000 points on the sphere at r = 0.065: %d kept" % kept)
    assert 500 < kept < 3000 and c["want"].sum() == kept


def test_ragged_batch_with_radii_and_a_validity_mask(dev):
    rng = np.random.RandomState(12)
    pts = np.stack([D.sphere_cloud(2048, 20 + n) for n in range(4)])
    lengths = [0, 1, 700, 2048]
    radii = [0.1, 0.3, 0.11, 0.07]
    got = run(dev, pts, radii, lengths)
    check(got, pts, radii, lengths)
    assert got[2].tolist()[:2] == [0, 1] and not got[0][0].any() and got[1][1, 0] == 0
    valid = rng.rand(4, 2048) > 0.1
    for v in (valid, valid.astype(np.uint8), valid.astype(np.float32)):
        got = run(dev, pts, radii, lengths, v)
        check(got, pts, radii, lengths, valid)
    assert not (got[0] & ~valid).any()


def test_duplicates_and_ties(dev):
    rng = np.random.RandomState(5)
    base = rng.rand(600, 3).astype(np.float32)
    pts = np.concatenate([base, base[::2], base[:100]])
    got = run(dev, pts, 1e-6)
    check(got, pts, 1e-6)
    assert got[0][0, :600].all() and not got[0][0, 600:].any()                    # the lower index of a duplicate is kept
    # pairs at exactly d2 == r2 conflict, pairs one ulp farther do not: along each axis, spread far apart
    r = np.float32(0.3)
    far = np.nextafter(r, np.float32(1.0))
    rows, keep = [], []
    for k, axis in enumerate((0, 1, 2, 0, 1, 2)):
        a = np.zeros(3, dtype=np.float32)
        a[(axis + 1) % 3] = 10.0 * (k + 1)                                        # the pairs lie far from one another
        b = a.copy()
        b[axis] = r if k < 3 else far                                             # from 0: the offset is the coordinate itself
        rows += [a, b]
        keep += [True, k >= 3]
    pts = np.stack(rows)
    got = run(dev, pts, float(r))
    check(got, pts, float(r))
    assert got[0][0].tolist() == keep


def test_chain_in_order_and_shuffled(dev):
    r = 0.05
    pts, _ = D.chain(257, r)
    got = run(dev, pts, r)
    check(got, pts, r)
    assert (np.nonzero(got[0][0])[0] == np.arange(0, 257, 2)).all()
    pts, order = D.chain(257, r, shuffle_seed=4)
    got = run(dev, pts, r)
    check(got, pts, r)


def test_reach_cells_smaller_than_the_radius(dev):
    from iso_points_amd import frnn
    pts = np.random.RandomState(13).rand(4000, 3).astype(np.float32)
    r = 0.25
    t = torch.from_numpy(pts[None]).to(dev)
    grid = frnn.build_grid(t, frnn._as_lengths(None, 1, 4000, dev), frnn._as_radius(r, 1, dev))
    cell = 1.0 / float(grid.params[0, 3])
    print("cell %.4f against r = %.2f" % (cell, r))
    assert cell < r
    got = run(dev, pts, r)
    check(got, pts, r)
    assert 10 < got[2][0] < 400


def test_reach_radius_below_every_distance_and_above_the_diagonal(dev):
    pts = np.random.RandomState(14).rand(1500, 3).astype(np.float32)
    d2 = ((pts[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(-1)
    d2[np.arange(1500), np.arange(1500)] = np.inf
    small = 0.5 * float(np.sqrt(d2.min()))
    got = run(dev, pts, small)
    check(got, pts, small)
    assert got[0].all() and got[2][0] == 1500 and (got[1][0] == np.arange(1500)).all()
    got = run(dev, pts, 2.0)                                                      # the unit cube's diagonal is 1.74
    check(got, pts, 2.0)
    assert got[2][0] == 1 and got[0][0, 0] and got[1][0].tolist() == [0] + [-1] * 1499


def test_results_do_not_depend_on_rounds_per_batch(dev, monkeypatch):
    from iso_points_amd import point_processing
    c = case1(dev)
    chain, _ = D.chain(257, 0.05)
    again = run(dev, c["pts"], 0.065)
    for a, b in zip(again, c["got"]):
        assert (a == b).all()
    ref_chain = run(dev, chain, 0.05)
    for batch in (1, 64):
        monkeypatch.setattr(point_processing, "ROUNDS_PER_BATCH", batch)
        for a, b in zip(run(dev, c["pts"], 0.065), c["got"]):
            assert (a == b).all(), batch
        for a, b in zip(run(dev, chain, 0.05), ref_chain):
            assert (a == b).all(), batch


def test_prefix_stability(dev):
    c = case1(dev)
    got = run(dev, c["pts"][:1000], 0.065)
    assert (got[0][0] == c["got"][0][0, :1000]).all()
    assert got[2][0] == c["got"][0][0, :1000].sum()


# ------------------------------------------------------------------------------------------------------------ the sampler
def as_tuple(dev, meshes):
    """(verts (N,V,3), faces (N,F,3), num_faces) of a list of (verts, faces) numpy pairs, padded."""
    N = len(meshes)
    V, F = max([len(v) for v, _ in meshes] + [1]), max([len(f) for _, f in meshes] + [1])
    verts, faces = torch.zeros(N, V, 3), torch.zeros(N, F, 3, dtype=torch.int64)
    for n, (v, f) in enumerate(meshes):
        verts[n, :len(v)] = torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(-1, 3)
        faces[n, :len(f)] = torch.from_numpy(np.asarray(f, dtype=np.int64)).reshape(-1, 3)
    return verts.to(dev), faces.to(dev), torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)


def gen(k):
    return torch.Generator().manual_seed(k)


def no_conflict_left(points, r):
    conf = D.conflicts(points, r)
    conf[np.arange(len(conf)), np.arange(len(conf))] = False
    return not conf.any()


@pytest.mark.parametrize("name,S", SAMPLER_CASES)
def test_sampler_equals_the_gather_of_the_uniform_draw(dev, name, S):
    from iso_points_amd.ops import sample_points_from_meshes, sample_points_from_meshes_even
    from iso_points_amd.point_processing import remove_close
    verts, faces = sampler_mesh(name)
    mesh = as_tuple(dev, [(verts, faces)])
    r = D.default_radius(verts, faces, S)
    for k in (1, 2, 3):
        pts, num, nrm, face, bary = sample_points_from_meshes_even(mesh, S, return_normals=True, return_faces=True,
                                                                   generator=gen(k))
        assert tuple(pts.shape) == (1, S, 3) and num.dtype == torch.int64 and face.dtype == torch.int64
        assert num.tolist() == [S]
        p3, n3, f3, b3 = sample_points_from_meshes(mesh, 3 * S, return_normals=True, return_faces=True, generator=gen(k))
        mask, sel, kept = remove_close(p3, float(r), valid=f3 >= 0)
        assert int(kept[0]) >= S
        # the elimination of the draw is the oracle's, on the bits the GPU drew
        m, s, kk = D.serial(p3[0].cpu().numpy(), r, valid=(f3[0] >= 0).cpu().numpy())
        assert (mask[0].cpu().numpy() == m).all() and (sel[0].cpu().numpy() == s).all() and int(kept[0]) == kk
        take = sel[0, :S]
        assert torch.equal(pts[0], p3[0, take]) and torch.equal(nrm[0], n3[0, take])
        assert torch.equal(face[0], f3[0, take]) and torch.equal(bary[0], b3[0, take])
        assert no_conflict_left(pts[0].cpu().numpy(), r)
        # the explicit radius is the default's value
        pts_r, num_r = sample_points_from_meshes_even(mesh, S, float(r), generator=gen(k))
        assert torch.equal(pts_r, pts) and torch.equal(num_r, num)


def test_sampler_first_rows_do_not_depend_on_oversample(dev):
    from iso_points_amd.ops import sample_points_from_meshes_even
    verts, faces = sampler_mesh("ico2")
    mesh = as_tuple(dev, [(verts, faces)])
    r = float(D.default_radius(verts, faces, 300))
    a = sample_points_from_meshes_even(mesh, 300, r, return_normals=True, return_faces=True, generator=gen(2), oversample=3)
    b = sample_points_from_meshes_even(mesh, 300, r, return_normals=True, return_faces=True, generator=gen(2), oversample=5)
    assert a[1].tolist() == [300] and b[1].tolist() == [300]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # too few draws: fewer than S points, the rows beyond are zero
    pts, num, face, _ = sample_points_from_meshes_even(mesh, 300, r, return_faces=True, generator=gen(2), oversample=1)
    k = int(num[0])
    assert 0 < k < 300 and torch.equal(pts[0, :k], a[0][0, :k])
    assert not pts[0, k:].any() and (face[0, k:] == -1).all() and (face[0, :k] >= 0).all()


def test_sampler_meshes_without_faces_or_area_yield_nothing(dev):
    from iso_points_amd.ops import sample_points_from_meshes_even
    verts, faces = sampler_mesh("ico2")
    flat = np.zeros_like(verts)
    flat[:, 0] = verts[:, 0]                                                      # every face collapsed onto a line
    mesh = as_tuple(dev, [(verts, faces), (verts, faces[:0]), (flat, faces), (verts, faces)])
    pts, num, nrm, face, bary = sample_points_from_meshes_even(mesh, 300, return_normals=True, return_faces=True,
                                                               generator=gen(3))
    assert num.tolist() == [300, 0, 0, 300]
    for n in (1, 2):
        assert not pts[n].any() and not nrm[n].any() and not bary[n].any() and (face[n] == -1).all()
    single = sample_points_from_meshes_even(as_tuple(dev, [(verts, faces)]), 300, generator=gen(3))
    assert torch.equal(single[0][0], pts[0])                                      # mesh 0 of the batch alone: the same points


def test_sampler_gradient_is_the_uniform_gradient_gathered(dev):
    from iso_points_amd.ops import sample_points_from_meshes, sample_points_from_meshes_even
    from iso_points_amd.point_processing import remove_close
    S = 500
    verts, faces = sampler_mesh("scaled")
    v0, f, num_f = as_tuple(dev, [(verts, faces)])
    r = float(D.default_radius(verts, faces, S))
    g = torch.Generator(device=dev).manual_seed(7)
    Wp, Wn = torch.randn(1, S, 3, generator=g, device=dev), torch.randn(1, S, 3, generator=g, device=dev)

    def even():
        v = v0.clone().requires_grad_(True)
        pts, num, nrm = sample_points_from_meshes_even((v, f, num_f), S, r, return_normals=True, generator=gen(1))
        assert num.tolist() == [S] and pts.requires_grad and nrm.requires_grad
        ((pts * Wp).sum() + (nrm * Wn).sum()).backward()
        return v.grad

    def by_hand():
        v = v0.clone().requires_grad_(True)
        p3, n3, f3, _ = sample_points_from_meshes((v, f, num_f), 3 * S, return_normals=True, return_faces=True, generator=gen(1))
        _, sel, _ = remove_close(p3.detach(), r, valid=f3 >= 0)
        take = sel[0, :S]
        ((p3[0, take] * Wp[0]).sum() + (n3[0, take] * Wn[0]).sum()).backward()
        return v.grad
    ga, gb, ga2 = even(), by_hand(), even()
    assert ga.abs().max() > 0 and torch.isfinite(ga).all()
    assert torch.equal(ga, gb) and torch.equal(ga, ga2)
