"""iso_points_amd.ops.sample_points_from_meshes / mesh_face_areas_normals on the GPU against the draw of
include/isopoints.h section I restated in numpy (tests/mesh_sample_oracle.py: Philox4x32-10, float32 areas, their float64
running sum C, the first face with C[f] > uf * A, the square-root weights) and float64 evaluations written here.

Face choice: equal to the oracle's wherever t = uf * A is farther than 1e-12 * A from every boundary of the oracle's C (the
kernel's C is the same sum in another fixed order: a few 1e-16 * A apart); at most 0.1 % of the samples may be excluded so.
Weights: the oracle's bit for bit (integer -> float conversions, one correctly rounded sqrt, two products, one subtraction).
Values and gradients: |got - ref| <= 1e-5 |ref| + A_tol against float64 at the returned faces and weights; A_tol is never
taken from the kernel: it is 4x the largest error of the same formula evaluated in float32 by torch on the CPU, computed
and printed by each test (the convention of tests/test_pfdist_gpu.py).

Meshes: the icosphere of level 2 scaled by (3, 1, 0.5) (320 faces, areas 1 : 3.6); a warped 200 x 200 grid = 80 000 faces:
the scan works in tiles of 2048 faces (256 threads x 8), so it spans 40 tiles, the last one partly filled, and one chain of
tile sums, and the draw's LDS table holds every 20th entry of its C (4 000 chunks; the meshes of up to 4 096 faces have a
stride of 1); a 260 x 260 grid = 135 200 faces = 67 tiles, past the 64 tile sums one chain step takes (table stride 34);
1 001 faces of which one has area ~ 1 and the others ~ 1e-8.  A generator seeded with k hands the call the seed O.seed_of(k)."""
import numpy as np
import pytest
import torch

import mesh_sample_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-5
EPS = 2.220446e-16
MESHES = {"ico": O.scaled_icosphere, "grid": O.warped_grid, "grid260": lambda: O.warped_grid(260), "wide": O.wide_range_mesh}


# ---------------------------------------------------------------------------------------------------------------- inputs
def as_tuple(dev, meshes):
    """(verts (N,V,3), faces (N,F,3), num_faces) of a list of (verts, faces) numpy pairs, padded."""
    N = len(meshes)
    V, F = max([len(v) for v, _ in meshes] + [1]), max([len(f) for _, f in meshes] + [1])
    verts, faces = torch.zeros(N, V, 3), torch.zeros(N, F, 3, dtype=torch.int64)
    for n, (v, f) in enumerate(meshes):
        verts[n, :len(v)] = torch.from_numpy(np.asarray(v, dtype=np.float32)).reshape(-1, 3)
        faces[n, :len(f)] = torch.from_numpy(np.asarray(f, dtype=np.int64)).reshape(-1, 3)
    return verts.to(dev), faces.to(dev), torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)


class StubMeshes(object):
    """What sample_points_from_meshes reads of a pytorch3d Meshes, from the same list."""

    def __init__(self, dev, meshes):
        off = np.cumsum([0] + [len(v) for v, _ in meshes])
        self.v = torch.from_numpy(np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])).to(dev)
        self.f = torch.from_numpy(np.concatenate([np.asarray(f, np.int64).reshape(-1, 3) + off[n]
                                                  for n, (_, f) in enumerate(meshes)])).to(dev)
        self.num = torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)

    def verts_packed(self):
        return self.v

    def faces_packed(self):
        return self.f.float()                      # evaluation.py:111 builds its Meshes from float faces

    def mesh_to_faces_packed_first_idx(self):
        return (torch.cumsum(self.num, 0) - self.num).to(self.v.device)

    def num_faces_per_mesh(self):
        return self.num.to(self.v.device)


def draw(dev, meshes, S, k, **kw):
    from iso_points_amd.ops import sample_points_from_meshes
    return sample_points_from_meshes(as_tuple(dev, meshes), S, generator=torch.Generator().manual_seed(k), **kw)


_ORACLE = {}


def oracle(name, k, n, S):
    key = (name, k, n, S)
    if key not in _ORACLE:
        v, f = MESHES[name]()
        _ORACLE[key] = O.sample(v[f], O.seed_of(k), n, S)
    return _ORACLE[key]


def check_choice(names, k, S, face_idx, bary, limit=1e-3):
    """face_idx and bary of a batch of the named meshes against the oracle; returns the number of excluded samples."""
    first, excluded = 0, 0
    for n, name in enumerate(names):
        d = oracle(name, k, n, S)
        got = face_idx[n].cpu().numpy() - first
        F = len(MESHES[name]()[1])
        assert got.min() >= 0 and got.max() < F, (name, got.min(), got.max())
        clear = d["margin"] > 1e-12 * d["A"]
        wrong = got[clear] != d["face"][clear]
        assert not wrong.any(), "%s: %d of %d faces differ from the oracle's" % (name, int(wrong.sum()), S)
        assert (np.abs(got - d["face"]) <= 1)[~clear].all()
        excluded += int((~clear).sum())
        assert np.array_equal(bary[n].cpu().numpy().view(np.uint32), d["bary"].view(np.uint32)), name
        first += F
    print("%s: %d of %d samples within 1e-12 A of a boundary" % (names, excluded, S * len(names)))
    assert excluded <= limit * S * len(names)
    return excluded


def close(got, ref, A):
    got, ref = got.detach().cpu().double(), ref.double()
    bad = (got - ref).abs() > REL * ref.abs() + A
    assert not bad.any(), "%d of %d beyond 1e-5 rel + %.3g: worst |d| = %.3g" % (
        int(bad.sum()), bad.numel(), A, (got - ref).abs().max().item())


# ------------------------------------------------------------------------------------------- the formulas, in any dtype
def cross3(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)


def areas_normals(tris):
    m = cross3(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    length = ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]).sqrt()
    return 0.5 * length, m / length.clamp(min=EPS)[:, None]


def points_normals(tris, face, bary):
    """Points and normals of samples at packed faces `face` with weights `bary`, in the dtype of tris."""
    t, w = tris[face], bary.to(tris.dtype)
    p = (w[:, 0:1] * t[:, 0] + w[:, 1:2] * t[:, 1]) + w[:, 2:3] * t[:, 2]
    return p, areas_normals(tris)[1][face]


def tol(fn):
    """(the float64 results of fn(dtype), 4x the largest error of its float32 CPU evaluation per result)."""
    r64, r32 = fn(torch.float64), fn(torch.float32)
    return r64, [4.0 * (a.double() - b).abs().max().item() for a, b in zip(r32, r64)]


# ------------------------------------------------------------------------------------------- 1. face choice and weights
@pytest.mark.parametrize("name", ["ico", "grid", "grid260", "wide"])
def test_face_choice_and_weights_equal_the_oracle(dev, name):
    S = 20000
    _, face_idx, bary = draw(dev, [MESHES[name]()], S, 1, return_faces=True)
    assert face_idx.dtype == torch.int64 and tuple(face_idx.shape) == (1, S) and tuple(bary.shape) == (1, S, 3)
    check_choice([name], 1, S, face_idx, bary)


def test_face_choice_in_a_batch_of_unequal_meshes(dev):
    """N = 3 with 1 001, 80 000 and 320 faces: mesh n draws with counter word n and searches its own rows of C."""
    names, S = ["wide", "grid", "ico"], 20000
    _, face_idx, bary = draw(dev, [MESHES[n]() for n in names], S, 2, return_faces=True)
    check_choice(names, 2, S, face_idx, bary)


def test_small_faces_next_to_a_large_one_are_reached(dev):
    """The wide-range mesh at S = 2 000 000: its 1 000 small faces hold 1e-5 of the area, so about 20 samples fall on them;
    a float32 running sum would step over every one of them behind the large face."""
    S = 2000000
    _, face_idx, bary = draw(dev, [O.wide_range_mesh()], S, 3, return_faces=True)
    check_choice(["wide"], 3, S, face_idx, bary)
    small = face_idx[0].cpu().numpy() != 500
    want = oracle("wide", 3, 0, S)["face"] != 500
    print("samples on the small faces: %d (oracle %d), behind the large one: %d" % (
        small.sum(), want.sum(), (face_idx[0].cpu().numpy() > 500).sum()))
    assert want.sum() >= 5 and small.sum() == want.sum() and (face_idx[0].cpu().numpy() > 500).sum() >= 1
    del _ORACLE[("wide", 3, 0, S)]


def test_more_meshes_than_one_grid_dimension_holds(dev):
    """65 600 meshes of one face each, one sample each: the mesh index runs past the 65 535 workgroups of the grid's second
    dimension.  Every sample lies on its own mesh's face with the weights of counter (0, 0, n, 0)."""
    from iso_points_amd.ops import sample_points_from_meshes
    N = 65600
    g = torch.Generator().manual_seed(4)
    verts = torch.rand(N, 3, 3, generator=g) + torch.arange(N, dtype=torch.float32)[:, None, None] * 0.01
    faces = torch.arange(3).repeat(N, 1, 1)
    points, face_idx, bary = sample_points_from_meshes((verts.to(dev), faces.to(dev)), 1, return_faces=True,
                                                       generator=torch.Generator().manual_seed(4))
    seed = O.seed_of(4)
    r = O.philox4x32_10((0, 0, np.arange(N), 0), (seed & O.MASK, (seed >> 32) & O.MASK))
    u = (r[2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    v = (r[3] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(bary[:, 0].cpu().numpy().view(np.uint32), O.bary32(u, v).view(np.uint32))
    assert torch.equal(face_idx[:, 0].cpu(), torch.arange(N))
    (p64, _), (A, _) = tol(lambda dt: points_normals(verts.to(dt), torch.arange(N), bary[:, 0].cpu()))
    close(points[:, 0], p64, A)


# ------------------------------------------------------------------------------------------------ 2. points and normals
@pytest.mark.parametrize("name", ["ico", "grid", "wide"])
def test_points_and_normals_against_float64(dev, name):
    """Points and normals against float64 at the returned faces and weights; normals have unit length within 1e-6; and every
    point lies on the mesh by the project's own search: nearest_faces gives d2 <= (1 + 1e-5) D2 + A_d2, where
    D2 = 3 (1e-5 max|p| + A_tol)^2 is what the first bound leaves per point and A_d2 is 4x the largest float32 CPU error of
    the distance formula (test_pfdist_gpu.pair_d2) on the pairs (point, its face)."""
    from iso_points_amd.loss import nearest_faces
    from test_pfdist_gpu import pair_d2
    S = 20000
    v, f = MESHES[name]()
    points, normals, face_idx, bary = draw(dev, [(v, f)], S, 1, return_normals=True, return_faces=True)
    tris = torch.from_numpy(v[f])
    face, w = face_idx[0].cpu(), bary[0].cpu()
    (p64, n64), (A_p, A_n) = tol(lambda dt: points_normals(tris.to(dt), face, w))
    print("%s: A points %.3g, normals %.3g" % (name, A_p, A_n))
    close(points[0], p64, A_p)
    close(normals[0], n64, A_n)
    assert ((normals[0].double().norm(dim=-1) - 1.0).abs() <= 1e-6).all()
    got = points[0].cpu()
    r64 = pair_d2(got.double(), tris.double()[face])
    A_d2 = 4.0 * (pair_d2(got, tris[face]).double() - r64).abs().max().item()
    D2 = 3.0 * (REL * p64.abs().max().item() + A_p) ** 2
    d2, _ = nearest_faces(points[0], tris.to(dev))
    print("%s: d2 max %.3g, D2 %.3g, A_d2 %.3g" % (name, d2.max().item(), D2, A_d2))
    assert r64.max().item() <= D2
    assert (d2 >= 0).all() and d2.max().item() <= (1.0 + REL) * D2 + A_d2


# ------------------------------------------------------------------------------------------------------ 3. distribution
def test_distribution_over_faces_and_inside_a_face(dev):
    """Scaled icosphere, S = 200 000, generator seeds 1, 2, 3, 12345: chi-square of the face counts against S * area / A over
    319 degrees of freedom below 319 + 6 sqrt(638) = 471; the three weight means within 5 sqrt(1/18 / S) of 1/3.  The
    inputs are fixed: this always passes or always fails (tests/test_mesh_sample_cpu.py holds the oracle to the same)."""
    S = 200000
    v, f = O.scaled_icosphere()
    areas = O.face_areas32(v[f])
    for k in (1, 2, 3, 12345):
        _, face_idx, bary = draw(dev, [(v, f)], S, k, return_faces=True)
        chi2 = O.chi_square(face_idx[0].cpu().numpy(), areas, S)
        means = bary[0].double().mean(dim=0).cpu().numpy()
        print("k = %d: chi-square %.1f, weight means - 1/3 %s" % (k, chi2, means - 1.0 / 3.0))
        assert chi2 < O.CHI2_BOUND
        assert (np.abs(means - 1.0 / 3.0) <= O.bary_mean_bound(S)).all()


# ------------------------------------------------------------------------------- 4. determinism and prefix stability
def test_determinism_and_prefix_stability(dev):
    from iso_points_amd.ops import sample_points_from_meshes
    ico, grid, wide = O.scaled_icosphere(), O.warped_grid(), O.wide_range_mesh()
    kw = dict(return_normals=True, return_faces=True)
    a = draw(dev, [ico, grid, wide], 4000, 5, **kw)
    b = draw(dev, [ico, grid, wide], 4000, 5, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the first 1 000 of 4 000 are the request for 1 000
    c = draw(dev, [ico, grid, wide], 1000, 5, **kw)
    for x, y in zip(a, c):
        assert torch.equal(x[:, :1000], y)
    # mesh 1 of another batch: the same samples (its packed rows start elsewhere)
    d = draw(dev, [wide, grid, ico], 4000, 5, **kw)
    assert torch.equal(a[0][1], d[0][1]) and torch.equal(a[1][1], d[1][1]) and torch.equal(a[3][1], d[3][1])
    assert torch.equal(a[2][1] - len(ico[1]), d[2][1] - len(wide[1]))
    # another seed differs
    e = draw(dev, [ico, grid, wide], 4000, 6, **kw)
    assert not torch.equal(a[0], e[0]) and not torch.equal(a[2], e[2])
    # the default generator: torch.manual_seed governs the call, and two calls in a row differ
    meshes = as_tuple(dev, [ico, grid])
    torch.manual_seed(7)
    p1, p2 = sample_points_from_meshes(meshes, 500), sample_points_from_meshes(meshes, 500)
    torch.manual_seed(7)
    q1, q2 = sample_points_from_meshes(meshes, 500), sample_points_from_meshes(meshes, 500)
    assert torch.equal(p1, q1) and torch.equal(p2, q2) and not torch.equal(p1, p2)
    assert tuple(p1.shape) == (2, 500, 3) and p1.dtype == torch.float32


def test_default_call_reads_nothing_back(dev):
    """No device-to-host read in a call on the tuple form without num_faces, backward included."""
    from iso_points_amd.ops import sample_points_from_meshes
    v, f = O.scaled_icosphere()
    verts = torch.from_numpy(v)[None].to(dev).requires_grad_(True)
    faces = torch.from_numpy(f)[None].to(dev)
    sample_points_from_meshes((verts, faces), 300, return_normals=True)[0].sum().backward()      # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        verts.grad = None
        p, n = sample_points_from_meshes((verts, faces), 300, return_normals=True)
        (p.sum() + n[..., 0].sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(verts.grad).all() and verts.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------------------ 5. edge shapes
def edge_batch():
    """No faces; one face; five faces without area (repeated vertices, collinear vertices with few bits); the scaled
    icosphere with 20 faces without area spliced in at every 17th row."""
    v, f = O.scaled_icosphere()
    spliced = []
    for i, row in enumerate(f.tolist()):
        if i % 16 == 0:
            spliced.append([row[0], row[0], row[1]])
        spliced.append(row)
    spliced = np.array(spliced, dtype=np.int64)
    assert len(spliced) == 340
    one = (np.array([[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.0, 1.0, 1.5]], np.float32), np.array([[0, 1, 2]]))
    flat_v = np.array([[0.5, 0.25, 1.25], [0.75, 0.5, 1.0], [-1.25, 0.5, 0.25], [-1.0, 0.75, 0.5], [-0.75, 1.0, 0.75]], np.float32)
    flat_f = np.array([[0, 0, 1], [1, 0, 0], [2, 3, 4], [4, 3, 2], [3, 3, 3]])
    return [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), one, (flat_v, flat_f), (v, spliced)]


def test_edge_shapes(dev):
    from iso_points_amd.ops import mesh_face_areas_normals, sample_points_from_meshes
    meshes, S = edge_batch(), 3000
    points, normals, face_idx, bary = draw(dev, meshes, S, 8, return_normals=True, return_faces=True)
    for n in (0, 2):
        assert not points[n].any() and not normals[n].any() and not bary[n].any() and (face_idx[n] == -1).all()
    assert (face_idx[1] == 0).all()
    # the spliced sphere: packed rows 6 .. 345, never a face without area, and the oracle's choice
    stub = StubMeshes(dev, meshes)
    areas, _ = mesh_face_areas_normals(stub.verts_packed(), stub.faces_packed().long())
    assert (areas[1:6] == 0).all() and (areas[6:] == 0).sum() == 20
    assert (face_idx[3] >= 6).all() and (face_idx[3] < 346).all() and (areas[face_idx[3]] > 0).all()
    v, f = meshes[3]
    d = O.sample(v[f], O.seed_of(8), 3, S)
    clear = d["margin"] > 1e-12 * d["A"]
    assert clear.mean() >= 0.999 and np.array_equal((face_idx[3].cpu().numpy() - 6)[clear], d["face"][clear])
    assert np.array_equal(bary[3].cpu().numpy().view(np.uint32), d["bary"].view(np.uint32))
    # the Meshes-like form is the tuple form
    again = sample_points_from_meshes(stub, S, return_normals=True, return_faces=True, generator=torch.Generator().manual_seed(8))
    for x, y in zip((points, normals, face_idx, bary), again):
        assert torch.equal(x, y)
    # S = 0
    empty = draw(dev, meshes, 0, 8, return_normals=True, return_faces=True)
    assert [tuple(x.shape) for x in empty] == [(4, 0, 3), (4, 0, 3), (4, 0), (4, 0, 3)]
    assert tuple(draw(dev, meshes, 0, 8).shape) == (4, 0, 3)
    # and a batch of nothing but empty meshes, with gradients asked for
    verts = torch.zeros(2, 3, 3, device=dev, requires_grad=True)
    p = sample_points_from_meshes((verts, torch.zeros(2, 0, 3, dtype=torch.int64, device=dev)), 10)
    assert tuple(p.shape) == (2, 10, 3) and not p.any()
    p.sum().backward()
    assert not verts.grad.any()


# ---------------------------------------------------------------------------------------------------------- 6. gradients
def grad_case(name):
    """Meshes whose faces have vertices of their own: verts.grad is then the triangles' gradient as the kernels wrote it."""
    if name == "ico":
        v, f = O.scaled_icosphere()
        tris = v[f]
    elif name == "two":
        tris = np.array([[[0.0, 0.0, 0.0], [1.5, 0.25, 0.0], [0.25, 1.0, 0.5]],
                         [[1.5, 0.25, 0.0], [1.75, 1.5, 0.75], [0.25, 1.0, 0.5]]], np.float32)
    else:
        tris = np.array([[[0.25, -0.5, 0.125], [1.5, 0.25, 0.0], [0.25, 1.0, 0.75]]], np.float32)
    return tris.reshape(-1, 3), np.arange(tris.shape[0] * 3).reshape(-1, 3)


@pytest.mark.parametrize("name,S", [("ico", 1000), ("two", 1200), ("one", 5000)])
def test_gradients_against_float64_autograd(dev, name, S):
    """The loss is a fixed random weighting of points and normals.  320 faces at S = 1 000: lists of a few samples, summed by
    their own lane; 2 faces at S = 1 200: lists of about 600, sorted by one wave; 1 face at S = 5 000: beyond 1 024, the
    strided path."""
    from iso_points_amd.ops import sample_points_from_meshes
    v, f = grad_case(name)
    g = torch.Generator().manual_seed(31)
    Wp, Wn = torch.randn(1, S, 3, generator=g), torch.randn(1, S, 3, generator=g)

    def run():
        verts = torch.from_numpy(v)[None].to(dev).requires_grad_(True)
        p, n, face_idx, bary = sample_points_from_meshes((verts, torch.from_numpy(f)[None].to(dev)), S, return_normals=True,
                                                         return_faces=True, generator=torch.Generator().manual_seed(9))
        assert p.requires_grad and n.requires_grad and not face_idx.requires_grad and not bary.requires_grad
        ((p * Wp.to(dev)).sum() + (n * Wn.to(dev)).sum()).backward()
        return verts.grad[0].clone(), face_idx[0].cpu(), bary[0].cpu()
    grad, face, w = run()
    again, _, _ = run()
    assert torch.equal(grad, again)
    counts = torch.bincount(face, minlength=len(f))
    print("%s: list lengths %d .. %d" % (name, counts.min(), counts.max()))
    if name == "ico":
        assert (counts <= 8).any() and (counts == 0).any()
    elif name == "two":
        assert ((counts > 8) & (counts <= 1024)).all()
    else:
        assert counts.max() > 1024

    def reference(dt):
        verts = torch.from_numpy(v).to(dt).requires_grad_(True)
        p, n = points_normals(verts[torch.from_numpy(f)], face, w)
        ((p * Wp[0].to(dt)).sum() + (n * Wn[0].to(dt)).sum()).backward()
        return [verts.grad]
    (g64,), (A,) = tol(reference)
    print("%s: A %.3g, largest |grad| %.3g" % (name, A, g64.abs().max().item()))
    close(grad, g64, A)
    # faces nobody chose: exactly zero
    unchosen = (counts == 0).repeat_interleave(3)
    assert not grad.cpu()[unchosen].any()
    # points alone: the normals' half is not computed and not missed
    verts = torch.from_numpy(v)[None].to(dev).requires_grad_(True)
    p = sample_points_from_meshes((verts, torch.from_numpy(f)[None].to(dev)), S, generator=torch.Generator().manual_seed(9))
    (p * Wp.to(dev)).sum().backward()

    def reference_points(dt):
        vv = torch.from_numpy(v).to(dt).requires_grad_(True)
        pp, _ = points_normals(vv[torch.from_numpy(f)], face, w)
        (pp * Wp[0].to(dt)).sum().backward()
        return [vv.grad]
    (g64,), (A,) = tol(reference_points)
    close(verts.grad[0], g64, A)


def test_gradient_through_shared_vertices_and_no_backward_without_a_request(dev):
    from iso_points_amd import _lib
    from iso_points_amd.ops import sample_points_from_meshes
    v, f = O.scaled_icosphere()
    faces = torch.from_numpy(f)[None].to(dev)
    S = 2000
    verts = torch.from_numpy(v)[None].to(dev).requires_grad_(True)
    p, n, face_idx, bary = sample_points_from_meshes((verts, faces), S, return_normals=True, return_faces=True,
                                                     generator=torch.Generator().manual_seed(10))
    g = torch.Generator().manual_seed(32)
    Wp, Wn = torch.randn(S, 3, generator=g), torch.randn(S, 3, generator=g)
    ((p[0] * Wp.to(dev)).sum() + (n[0] * Wn.to(dev)).sum()).backward()

    def reference(dt):
        vv = torch.from_numpy(v).to(dt).requires_grad_(True)
        pp, nn = points_normals(vv[torch.from_numpy(f)], face_idx[0].cpu(), bary[0].cpu())
        ((pp * Wp.to(dt)).sum() + (nn * Wn.to(dt)).sum()).backward()
        return [vv.grad]
    (g64,), (A,) = tol(reference)
    print("shared vertices: A %.3g" % A)
    close(verts.grad[0], g64, A)
    # vertices that ask for nothing: nothing is differentiable and nothing is kept for a backward pass
    out = sample_points_from_meshes((verts.detach(), faces), S, return_normals=True)
    assert not out[0].requires_grad and not out[1].requires_grad
    assert "iso_mesh_sample_backward" in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------- 7. mesh_face_areas_normals
@pytest.mark.parametrize("name", ["ico", "wide"])
def test_mesh_face_areas_normals_against_float64(dev, name):
    from iso_points_amd.ops import mesh_face_areas_normals
    v, f = MESHES[name]()
    areas, normals = mesh_face_areas_normals(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
    assert tuple(areas.shape) == (len(f),) and tuple(normals.shape) == (len(f), 3)
    (a64, n64), (A_a, A_n) = tol(lambda dt: areas_normals(torch.from_numpy(v[f]).to(dt)))
    print("%s: A areas %.3g, normals %.3g; areas %.3g .. %.3g" % (name, A_a, A_n, a64.min().item(), a64.max().item()))
    close(areas, a64, A_a)
    close(normals, n64, A_n)
    # and the areas are the oracle's bits: the face choice rests on that
    assert np.array_equal(areas.cpu().numpy().view(np.uint32), O.face_areas32(v[f]).view(np.uint32))
