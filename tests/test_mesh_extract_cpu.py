"""The numpy restatement of marching tetrahedra (tests/mesh_extract_oracle.py) checked by properties that do not depend on
it, without a GPU: tests/test_mesh_extract_gpu.py compares the kernels with it element for element, so a restatement that
is wrong in the way a kernel is wrong must fail here."""
import math

import numpy as np
import pytest

import mesh_extract_oracle as M


def _sphere(n=17, radius=0.6):
    shape, org, spc = M.box_grid(n)
    return M.volume(lambda p: M.sphere_sdf(p, radius), shape, org, spc), org, spc


def _torus(n=24):
    shape, org, spc = M.box_grid(n)
    return M.volume(lambda p: M.torus_sdf(p, 0.5, 0.2), shape, org, spc), org, spc


@pytest.fixture(scope="module")
def sphere():
    vol, org, spc = _sphere()
    return (vol, org, spc) + M.extract(vol, org, spc)


@pytest.fixture(scope="module")
def torus():
    vol, org, spc = _torus()
    return (vol, org, spc) + M.extract(vol, org, spc)


def test_the_six_tetrahedra_tile_the_cell():
    """Volumes 1/6 each with the sign of the permutation, and every shared face diagonal is the one that starts at the
    lower corner: 0 -> a+b for each pair of axes, so neighbouring cells agree."""
    total = 0.0
    for perm in M.PERMS:
        c = np.array(M.tet_corners(perm), dtype=np.float64)
        det = np.linalg.det(c[1:] - c[0])
        assert np.sign(det) == M._perm_sign(perm) and abs(abs(det) - 1.0) < 1e-12
        total += abs(det) / 6
        for u in range(4):
            for v in range(u + 1, 4):
                assert tuple(c[v] - c[u]) in [tuple(map(float, s)) for s in M.SLOTS]     # every edge is an owned slot
    assert abs(total - 1.0) < 1e-12
    # a point strictly inside the cell lies in exactly one tetrahedron: the one that sorts its coordinates
    rng = np.random.default_rng(0)
    for p in rng.random((50, 3)):
        hits = 0
        for perm in M.PERMS:
            c = np.array(M.tet_corners(perm), dtype=np.float64)
            lam = np.linalg.solve(np.vstack([c.T, np.ones(4)]), np.append(p, 1.0))
            hits += bool((lam > 0).all())
        assert hits == 1


def test_sixteen_cases_by_geometry():
    """Every case of tet_triangles on a real tetrahedron of either orientation: the triangles' corners lie on edges that
    join an inside to an outside corner, and each normal points from the inside corners to the outside ones."""
    for perm in M.PERMS:
        c = np.array(M.tet_corners(perm), dtype=np.float64)
        for m in range(16):
            inside = [bool(m >> q & 1) for q in range(4)]
            tris = M.tet_triangles(inside, M._perm_sign(perm))
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(inside)]
            val = np.where(inside, -1.0, 2.0)                        # linear field: the cut is at t = 1/3
            grad = np.linalg.solve(np.hstack([c, np.ones((4, 1))]), val)[:3]
            for tri in tris:
                pts = []
                for u, v in tri:
                    assert u < v and inside[u] != inside[v]
                    t = (0.0 - val[u]) / (val[v] - val[u])
                    pts.append(c[u] + t * (c[v] - c[u]))
                n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                assert np.linalg.norm(n) > 1e-3
                assert n @ grad > 0.999 * np.linalg.norm(n) * np.linalg.norm(grad)    # parallel to the gradient, same way
            if len(tris) == 2:                                       # the two halves of the quad share its diagonal
                assert len(set(tris[0]) & set(tris[1])) == 2 and len(set(tris[0]) | set(tris[1])) == 4


@pytest.mark.parametrize("which,chi", [("sphere", 2), ("torus", 0)])
def test_closed_oriented_and_euler(which, chi, request):
    _vol, _o, _s, verts, faces = request.getfixturevalue(which)
    assert len(faces) > 500
    assert M.is_closed_and_oriented(faces)
    assert M.euler_characteristic(faces) == chi
    assert sorted(np.unique(faces)) == list(range(len(verts)))      # every vertex is used, none is missing
    assert len(np.unique(M.components(faces))) == 1


def test_two_spheres_are_two_components():
    shape, org, spc = M.box_grid(26, 2.2)
    verts, faces = M.extract(M.volume(M.two_spheres_sdf, shape, org, spc), org, spc)
    lab = M.components(faces)
    assert M.is_closed_and_oriented(faces) and M.euler_characteristic(faces) == 4 and len(np.unique(lab)) == 2
    _n, area = M.face_normals_areas(verts, faces)
    a = [area[lab == c].sum() for c in (0, 1)]
    big = int(np.argmax(a))
    assert abs(verts[np.unique(faces[lab == big])].mean(0)[0] + 0.4) < 0.02       # the larger one sits at x = -0.4


@pytest.mark.parametrize("which", ["sphere", "torus"])
def test_normals_point_along_the_analytic_gradient(which, request):
    _vol, _o, _s, verts, faces = request.getfixturevalue(which)
    n, area = M.face_normals_areas(verts, faces)
    cen = verts[faces].astype(np.float64).mean(1)
    grad = cen / np.linalg.norm(cen, axis=1, keepdims=True) if which == "sphere" else M.torus_grad(cen, 0.5, 0.2)
    keep = area > 0
    assert keep.sum() > 500 and ((n[keep] * grad[keep]).sum(1) > 0).all()


@pytest.mark.parametrize("which", ["sphere", "torus"])
def test_vertices_lie_on_edges_at_the_linear_zero(which, request):
    """Every vertex is on a grid edge or diagonal that starts at its owner (at most one cell wide along every axis, two
    coordinates at most off the lattice in lockstep), within the linear-interpolation error of the field: for a distance
    field |f''| <= 1/rho along a line, rho the smallest radius of curvature met, so |f(v)| <= L^2 / (8 rho), L the edge."""
    vol, org, spc, verts, _faces = request.getfixturevalue(which)
    sdf = (lambda p: M.sphere_sdf(p, 0.6)) if which == "sphere" else (lambda p: M.torus_sdf(p, 0.5, 0.2))
    L = math.sqrt(3) * spc[0]
    rho = 0.6 - L if which == "sphere" else 0.2 - L
    assert np.abs(sdf(verts)).max() <= L * L / (8 * rho) + 1e-6
    frac = (verts.astype(np.float64) - np.array(org)) / np.array(spc)
    off = np.abs(frac - np.round(frac)) > 1e-4
    t = frac - np.floor(frac)
    for row_off, row_t in zip(off, t):
        assert row_off.any() and np.ptp(row_t[row_off]) < 1e-4      # the off-lattice coordinates share one t
    assert len(np.unique(verts, axis=0)) == len(verts)              # one vertex per active edge: nothing to weld


def test_vertex_order_is_point_then_slot():
    vol, org, spc, verts, _faces = _sphere(9) + M.extract(*_sphere(9))
    ins = M.inside_mask(vol, 0.0)
    n = vol.shape[0]
    want = []
    for p in range(n ** 3):
        i, j, k = p // (n * n), p // n % n, p % n
        for d in M.SLOTS:
            b = (i + d[0], j + d[1], k + d[2])
            if max(b) < n and ins[i, j, k] != ins[b]:
                want.append((i, j, k) + d)
    assert len(want) == len(verts)
    for (i, j, k, dx, dy, dz), v in zip(want, verts):                # the vertex lies inside its slot's box
        lo = np.array(org) + np.array([i, j, k]) * spc[0] - 1e-6
        hi = lo + np.array([dx, dy, dz]) * spc[0] + 2e-6
        assert (v >= lo).all() and (v <= hi).all()


def test_float32_and_float64_modes_agree():
    vol, org, spc = _sphere()
    v32, f32 = M.extract(vol, org, spc)
    v64, f64 = M.extract(vol, org, spc, dtype=np.float64)
    assert v32.dtype == np.float32 and v64.dtype == np.float64 and (f32 == f64).all()
    assert np.abs(v32 - v64).max() < 4e-7                           # a few ulp of coordinates below 1


def test_sphere_area_converges():
    r = 0.6
    err = []
    for n in (17, 33):
        vol, org, spc = _sphere(n, r)
        v, f = M.extract(vol, org, spc, dtype=np.float64)
        err.append(abs(M.face_normals_areas(v, f)[1].sum() / (4 * math.pi * r * r) - 1))
    print("relative area error of the float64 restatement, sphere r = 0.6: 17^3 %.3e, 33^3 %.3e" % tuple(err))
    assert err[1] < err[0] / 3 and err[1] < 5e-3                     # second order in the spacing


def test_level_and_ragged_grid():
    shape, org, spc = (5, 9, 70), (-0.6, -0.4, -0.7), (0.3, 0.1, 0.02)
    vol = M.volume(lambda p: M.sphere_sdf(p, 0.25), shape, org, spc)
    for level in (0.0, 0.1):
        v, f = M.extract(vol, org, spc, level=level)
        assert M.is_closed_and_oriented(f) and M.euler_characteristic(f) == 2
        # |p| - R is convex: a chord lies above it, so the chord's zero is never outside the level set; the x spacing is
        # close to the radius here, so it may be inside by a chord's sagitta
        r = np.linalg.norm(v.astype(np.float64), axis=1)
        assert r.max() <= 0.25 + level + 1e-6 and r.min() > 0.6 * (0.25 + level)


def test_values_on_the_level_count_as_outside():
    """x - 0.25 on a grid with points at x = 0.25: those points are outside, the vertices of their edges coincide with them
    (t = 0 or 1 exactly), the faces they span have no area and stay in the list."""
    shape, org, spc = (9, 4, 5), (-1.0, 0.0, 0.0), (0.25, 0.25, 0.25)
    vol = M.volume(lambda p: p[..., 0] - 0.25, shape, org, spc)
    assert (vol[5] == 0).all()
    v, f = M.extract(vol, org, spc)
    assert np.isfinite(v).all() and (v[:, 0] == 0.25).all()
    _n, area = M.face_normals_areas(v, f)
    assert (area == 0).any() and (area > 0).any()
    assert abs(area.sum() - 0.75 * 1.0) < 1e-6                       # the plane's patch inside the grid, counted once


def test_empty_and_non_finite():
    ones = np.ones((4, 5, 6), dtype=np.float32)
    for vol in (ones, -ones):
        v, f = M.extract(vol)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    shape, org, spc = M.box_grid(12)
    vol = M.volume(lambda p: M.sphere_sdf(p, 0.6), shape, org, spc)
    vol[:, 6, :] = np.nan
    vol[3, :, 2] = -np.inf
    v, f = M.extract(vol, org, spc)
    assert np.isfinite(v).all() and len(f) > 0                       # non-finite ends are never interpolated
    census = M.edge_census(f)
    assert all(c in ([1, 1], [1, 0], [0, 1]) for c in census.values())


def test_cut_by_the_box_is_open_only_on_the_box():
    shape, org, spc = M.box_grid(13)
    vol = M.volume(lambda p: M.sphere_sdf(p, 1.2), shape, org, spc)
    v, f = M.extract(vol, org, spc)
    open_edges = [e for e, c in M.edge_census(f).items() if c != [1, 1]]
    assert open_edges
    for (a, b) in open_edges:
        assert sorted(M.edge_census(f)[(a, b)]) == [0, 1]
        on_a, on_b = np.isclose(np.abs(v[a]), 1.0, atol=1e-6), np.isclose(np.abs(v[b]), 1.0, atol=1e-6)
        assert (on_a & on_b).any()                                   # both ends on one box face
