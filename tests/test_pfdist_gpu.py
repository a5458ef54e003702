"""iso_points_amd.loss.point_face_distance / face_point_distance / point_mesh_face_distance / nearest_faces on the GPU
against a brute force written here: pair_d2() evaluates the closest-point formula of include/isopoints.h section H for
every (point, face) pair in float64; torch autograd of the same function at the selected pairs gives the gradients.

Bound for a value: |d2 - ref| <= 1e-5 ref + A, and the same form for a gradient entry.  A is not chosen in advance and
never comes from the kernel: tol_values() / tol_grads() evaluate the same formula in float32 with torch on the CPU on the
inputs of the test at hand, take the largest error against float64 and give it a margin of 4x.  Measured on the CPU
for the cases below (largest float32 error -> A):
    values  shell cloud / icosphere 1280          point -> face 1.2e-08 -> 4.6e-08   face -> point 1.0e-08 -> 4.1e-08
    values  cube cloud / shrunken icosphere 1280  point -> face 7.0e-07 -> 2.8e-06   face -> point 2.4e-08 -> 9.7e-08
    grads   shell cloud / shrunken icosphere 320  point -> face 2.7e-07 -> 1.1e-06 (points), 2.4e-07 -> 9.4e-07 (tris)
                                                  face -> point 1.9e-07 -> 7.5e-07 (points), 1.2e-07 -> 5.0e-07 (tris)
(d2 is about 2.5e-3 in the shell case and up to 6 in the cube case, the gradients' entries are of order 0.1 to 1.)
An index is compared only where the float64 best and second best differ by more than 1e-5 relative (faces that share an
edge tie exactly in mathematics); at most 5 % of the queries of the two value cases may be excluded this way."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 1e-5


# ------------------------------------------------------------------------------------------------------------ the oracle
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_d2(p, tris, min_area=0.0):
    """Squared distance from p (..., 3) to the closed triangles tris (..., 3, 3) (broadcast), in the dtype of the inputs:
    |p - (b0 v0 + b1 v1 + b2 v2)|^2 at the plane projection where the area exceeds min_area and no weight is negative,
    otherwise the smallest over the three edges (01, 12, 20; the first of equals)."""
    v0, v1, v2 = tris[..., 0, :], tris[..., 1, :], tris[..., 2, :]

    def at(b0, b1, b2):
        r = p - ((b0[..., None] * v0 + b1[..., None] * v1) + b2[..., None] * v2)
        return dot3(r, r)

    def edge_t(a, b):
        d = b - a
        dd = dot3(d, d)
        t = dot3(p - a, d) / torch.where(dd > 0, dd, torch.ones_like(dd))
        return torch.where(dd > 0, t.clamp(0.0, 1.0), torch.zeros_like(t))
    e1, e2 = v1 - v0, v2 - v0
    n = torch.cross(e1, e2, dim=-1)
    nn = dot3(n, n)
    w = p - v0
    safe = torch.where(nn > 0, nn, torch.ones_like(nn))
    b1 = dot3(torch.cross(w, e2.expand_as(w), dim=-1), n) / safe
    b2 = dot3(torch.cross(e1.expand_as(w), w, dim=-1), n) / safe
    b0 = (1.0 - b1) - b2
    inside = (0.5 * nn.sqrt() > min_area) & (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
    zero = torch.zeros_like(b0)
    t01, t12, t20 = edge_t(v0, v1), edge_t(v1, v2), edge_t(v2, v0)
    d01, d12, d20 = at(1.0 - t01, t01, zero), at(zero, 1.0 - t12, t12), at(t20, zero, 1.0 - t20)
    best = d01
    best = torch.where(d12 < best, d12, best)
    best = torch.where(d20 < best, d20, best)
    return torch.where(inside, at(b0, b1, b2), best)


def all_pairs(points, tris, min_area=0.0, dtype=torch.float64):
    """(P, T) matrix on the CPU."""
    return pair_d2(points.to(dtype)[:, None, :], tris.to(dtype)[None], min_area)


def clear(d, dim):
    """Rows (dim=1) or columns (dim=0) of the float64 matrix whose best and second best differ by more than 1e-5 relative."""
    if d.shape[dim] < 2:
        return torch.ones(d.shape[1 - dim], dtype=torch.bool)
    two = d.topk(2, dim=dim, largest=False).values
    a, b = (two[:, 0], two[:, 1]) if dim == 1 else (two[0], two[1])
    return (b - a) > REL * b


def tol_values(points, tris, min_area, d64):
    """A of the two directions (point -> face, face -> point): 4x the largest error of the float32 CPU evaluation of the
    formula against the float64 matrix d64."""
    d32 = all_pairs(points, tris, min_area, torch.float32).double()
    return [4.0 * (d32.min(dim=dim).values - d64.min(dim=dim).values).abs().max().item() for dim in (1, 0)]


def close_both(d_p, d_t, points, tris, min_area, d64):
    A_p, A_t = tol_values(points, tris, min_area, d64)
    print("A: point -> face %.3g, face -> point %.3g" % (A_p, A_t))
    close(d_p, d64.min(dim=1).values, A_p)
    close(d_t, d64.min(dim=0).values, A_t)
    return A_p, A_t


def grads_at(points, tris, idx, w, direction, min_area, dtype):
    """Autograd of sum_q w_q d2(q, idx_q) with the indices fixed: (grad points, grad tris) on the CPU in `dtype`."""
    p = points.detach().cpu().to(dtype).requires_grad_(True)
    t = tris.detach().cpu().to(dtype).requires_grad_(True)
    idx, w = idx.cpu(), w.detach().cpu().to(dtype)
    ok = idx >= 0
    q = torch.nonzero(ok)[:, 0]
    if direction == 0:
        d2 = pair_d2(p[q], t[idx[q]], min_area)
    else:
        d2 = pair_d2(p[idx[q]], t[q], min_area)
    (w[q] * d2).sum().backward()
    return p.grad, t.grad


def close(got, ref, A):
    got, ref = got.detach().cpu().double(), ref.double()
    bad = (got - ref).abs() > REL * ref.abs() + A
    assert not bad.any(), "%d of %d beyond 1e-5 rel + %.3g: worst |d| = %.3g" % (
        int(bad.sum()), bad.numel(), A, (got - ref).abs().max().item())


# ------------------------------------------------------------------------------------------------------------ the meshes
def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = torch.tensor([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                      [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=torch.float64)
    f = torch.tensor([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                      [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                      [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    return v / v.norm(dim=1, keepdim=True), f


_SPHERES = {}


def icosphere(level):
    """(verts (V,3) f32, faces (F,3) long) of the unit icosphere after `level` subdivisions: 20 * 4^level faces."""
    if level not in _SPHERES:
        v, f = icosahedron()
        for _ in range(level):
            verts, mid, faces = [x for x in v], {}, []

            def midpoint(a, b):
                key = (min(a, b), max(a, b))
                if key not in mid:
                    m = verts[a] + verts[b]
                    verts.append(m / m.norm())
                    mid[key] = len(verts) - 1
                return mid[key]
            for a, b, c in f.tolist():
                ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
                faces += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
            v, f = torch.stack(verts), torch.tensor(faces)
        _SPHERES[level] = (v.float(), f)
    return _SPHERES[level]


def sphere_tris(level, radius=1.0, shrink=1.0, centre=(0.0, 0.0, 0.0)):
    """(F,3,3) f32 triangles; shrink < 1 pulls every face toward its own centroid, so that no two faces share an edge."""
    v, f = icosphere(level)
    tris = v[f] * radius
    c = tris.mean(dim=1, keepdim=True)
    return (c + (tris - c) * shrink + torch.tensor(centre)).contiguous()


def shell_cloud(P, seed):
    """Directions at random, radii 0.95 and 1.05 in turn."""
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    r = torch.where(torch.arange(P) % 2 == 0, torch.tensor(0.95), torch.tensor(1.05))
    return d * r[:, None]


def cube_cloud(P, seed, half=2.0):
    return (torch.rand(P, 3, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0) * half


def one(dev, n):
    return torch.zeros(1, dtype=torch.int64, device=dev), n


def both_directions(dev, points, tris, min_area=0.0):
    """The four results of one cloud against one mesh."""
    from iso_points_amd.loss import face_point_distance, nearest_faces, point_face_distance
    p, t = points.to(dev), tris.to(dev)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    d_p, i_p = nearest_faces(p, t, min_triangle_area=min_area)
    assert torch.equal(d_p, point_face_distance(p, first, t, first, p.shape[0], min_area))
    d_t = face_point_distance(p, first, t, first, p.shape[0], min_area)
    return d_p, i_p, d_t


_CASES = {}


def case(name):
    """The inputs of the two value cases and their float64 pair matrix, computed once."""
    if name not in _CASES:
        if name == "shell":
            points, tris = shell_cloud(2000, 11), sphere_tris(3)
        else:
            points, tris = cube_cloud(2000, 12), sphere_tris(3, shrink=0.8)
        _CASES[name] = (points, tris, all_pairs(points, tris))
    return _CASES[name]


# ------------------------------------------------------------------------------------------- 1. values and indices
@pytest.mark.parametrize("name", ["shell", "cube"])
def test_values_and_indices_both_directions(dev, name):
    """2000 points around a 1280-face icosphere: at radii 0.95 and 1.05 of the closed sphere ("shell"), and in the cube
    [-2, 2]^3 around the sphere with every face shrunk to 0.8 about its centroid ("cube": points outside the grid box and
    walks that pass kRingCap into the wave path; a far point of a CLOSED sphere is nearest to a shared edge or vertex
    more often than not, which is a tie, so this case takes the faces apart).  Every d2 is compared; an index where the
    float64 best and second best are more than 1e-5 relative apart, which may exclude at most 5 % of the queries."""
    points, tris, d64 = case(name)
    d_p, i_p, d_t = both_directions(dev, points, tris)
    close_both(d_p, d_t, points, tris, 0.0, d64)
    ok_p, ok_t = clear(d64, 1), clear(d64, 0)
    print("%s: clear %.4f of the points, %.4f of the faces" % (name, ok_p.float().mean(), ok_t.float().mean()))
    assert ok_p.float().mean() >= 0.95 and ok_t.float().mean() >= 0.95
    assert torch.equal(i_p.cpu()[ok_p], d64.argmin(dim=1)[ok_p])
    # the face -> point index is internal to the loss: read it from the search itself
    from iso_points_amd import loss
    pts, tr, seg = loss._pf_inputs(points.to(dev), one(dev, 0)[0], tris.to(dev), one(dev, 0)[0], None, 0.0, "test")
    _, i_t, _ = loss._pf_search(1, pts, tr, seg, 0.0)
    assert torch.equal(i_t.cpu().long()[ok_t], d64.argmin(dim=0)[ok_t])


def test_one_face_larger_than_a_cell(dev):
    """One triangle through the whole object is added to the fine sphere: R_max exceeds the grid's cells many times, every
    walk runs on until the reach less R_max covers its best, and the results are still the oracle's; the points near the
    centre choose the large face."""
    big = torch.tensor([[[-1.5, -1.2, 0.02], [1.5, -1.2, 0.01], [0.0, 1.6, -0.03]]])
    tris = torch.cat([sphere_tris(3)[:700], big, sphere_tris(3)[700:]])
    points = cube_cloud(1500, 13, half=1.2)
    d64 = all_pairs(points, tris)
    d_p, i_p, d_t = both_directions(dev, points, tris)
    close_both(d_p, d_t, points, tris, 0.0, d64)
    ok = clear(d64, 1)
    assert torch.equal(i_p.cpu()[ok], d64.argmin(dim=1)[ok])
    chose_big = (i_p.cpu() == 700) & ok
    assert chose_big.sum() > 100 and (d64.argmin(dim=1)[ok] == 700).sum() == chose_big.sum()


# ------------------------------------------------------------------------------------------- 2. degenerate input
def test_faces_without_area_among_normal_faces(dev):
    """A face with a repeated vertex and one with three collinear vertices (coordinates with few bits: their normal is
    exactly zero in float32 and in float64) among the faces of a sphere: finite values, equal to the oracle's."""
    tris = sphere_tris(2).clone()
    tris[17] = torch.tensor([[0.5, 0.25, 1.25], [0.5, 0.25, 1.25], [0.75, 0.5, 1.0]])
    tris[201] = torch.tensor([[-1.25, 0.5, 0.25], [-1.0, 0.75, 0.5], [-0.75, 1.0, 0.75]])
    points = torch.cat([shell_cloud(800, 14) * 1.1, torch.tensor([[0.6, 0.4, 1.2], [-1.0, 0.8, 0.6], [-1.5, 0.25, 0.0]])])
    d64 = all_pairs(points, tris)
    d_p, i_p, d_t = both_directions(dev, points, tris)
    assert torch.isfinite(d_p).all() and torch.isfinite(d_t).all()
    close_both(d_p, d_t, points, tris, 0.0, d64)
    assert i_p[800].item() == 17 and i_p[801].item() == 201 and i_p[802].item() == 201
    # and a mesh of nothing but such faces
    flat = torch.stack([tris[17], tris[201], tris[17] + 1.0])
    d_p, _, d_t = both_directions(dev, points, flat)
    f64 = all_pairs(points, flat)
    close_both(d_p, d_t, points, flat, 0.0, f64)


def test_points_on_a_vertex_an_edge_and_a_face(dev):
    """d2 == 0 exactly and a zero gradient for points that lie on the mesh (coordinates with few bits, so that the
    closest point is the point itself in float32)."""
    from iso_points_amd.loss import point_face_distance
    tris = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
                         [[2.0, 0.0, 1.0], [2.0, 2.0, 1.0], [4.0, 0.0, 1.0]],
                         [[0.0, 0.0, 3.0], [0.0, 1.0, 3.0], [1.0, 0.0, 3.0]]])
    points = torch.tensor([[0.0, 1.0, 0.0],      # a vertex of face 0
                           [0.5, 0.0, 0.0],      # the middle of an edge of face 0
                           [3.0, 1.0, 1.0],      # the middle of the long edge of face 1
                           [2.5, 0.5, 1.0],      # inside face 1
                           [0.25, 0.5, 3.0]])    # inside face 2
    p = points.to(dev).requires_grad_(True)
    t = tris.to(dev).requires_grad_(True)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    d2 = point_face_distance(p, first, t, first, 5)
    assert torch.equal(d2.detach().cpu(), torch.zeros(5))
    d2.sum().backward()
    assert torch.equal(p.grad.cpu(), torch.zeros(5, 3)) and torch.equal(t.grad.cpu(), torch.zeros(3, 3, 3))


def test_min_triangle_area_of_newer_pytorch3d(dev):
    """min_triangle_area = 5e-3: the faces of the unit sphere (area ~ 9.8e-3) keep their interior, those of a sphere of
    radius 0.6 inside it (~ 3.5e-3) are measured by their edges; against the oracle under the same rule."""
    tris = torch.cat([sphere_tris(3), sphere_tris(3, radius=0.6)])
    n = torch.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0], dim=-1).norm(dim=-1) * 0.5
    assert (n[:1280] > 7e-3).all() and (n[1280:] < 4.5e-3).all()
    points = torch.cat([shell_cloud(800, 15), shell_cloud(800, 16) * 0.6])
    d64 = all_pairs(points, tris, 5e-3)
    assert (d64.min(dim=1).values - all_pairs(points, tris).min(dim=1).values).abs().max() > 1e-4   # the rule matters
    d_p, i_p, d_t = both_directions(dev, points, tris, 5e-3)
    close_both(d_p, d_t, points, tris, 5e-3, d64)
    ok = clear(d64, 1)
    assert torch.equal(i_p.cpu()[ok], d64.argmin(dim=1)[ok])


# ------------------------------------------------------------------------------------------------------- 3. ties
def test_ties_go_to_the_lower_index(dev):
    from iso_points_amd import loss
    tris = sphere_tris(2, shrink=0.8).clone()
    tris[250] = tris[31]                                     # two coincident faces
    points = torch.cat([shell_cloud(600, 17), tris[31].mean(dim=0) * torch.tensor([[1.05], [0.97], [1.1]])])
    j = int(all_pairs(points, tris).argmin(dim=0)[100])       # the point face 100 is nearest to, a second time
    points = torch.cat([points, points[j:j + 1]])
    d64 = all_pairs(points, tris)
    _, i_p = loss.nearest_faces(points.to(dev), tris.to(dev))
    nearest = d64.argmin(dim=1)
    chose = (nearest == 31) | (nearest == 250)
    assert chose.sum() >= 3 and (i_p.cpu()[chose] == 31).all()
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    pts, tr, seg = loss._pf_inputs(points.to(dev), first, tris.to(dev), first, None, 0.0, "test")
    _, i_t, _ = loss._pf_search(1, pts, tr, seg, 0.0)
    nearest = d64.argmin(dim=0)
    chose = (nearest == j) | (nearest == points.shape[0] - 1)
    assert chose.sum() >= 1 and (i_t.cpu()[chose] == j).all()


# ---------------------------------------------------------------------------------------------------- 4. ragged batch
def ragged():
    """Three meshes and clouds of different sizes, one cloud with a single point and one mesh with a single face."""
    meshes = [sphere_tris(2, shrink=0.9), sphere_tris(0, radius=0.5, centre=(3.0, 0.0, 0.0))[4:5],
              sphere_tris(1, centre=(0.0, -2.0, 1.0), shrink=0.9)]
    clouds = [shell_cloud(500, 18), cube_cloud(300, 19) + torch.tensor([3.0, 0.0, 0.0]),
              torch.tensor([[0.1, -2.2, 2.3]])]
    return meshes, clouds


def test_ragged_batch_packed_and_reduced(dev):
    from iso_points_amd.loss import face_point_distance, point_face_distance, point_mesh_face_distance
    meshes, clouds = ragged()
    tris, points = torch.cat(meshes), torch.cat(clouds)
    t_len, p_len = [m.shape[0] for m in meshes], [c.shape[0] for c in clouds]
    t_first = torch.tensor([0, t_len[0], t_len[0] + t_len[1]], device=dev)
    p_first = torch.tensor([0, p_len[0], p_len[0] + p_len[1]], device=dev)
    d_p = point_face_distance(points.to(dev), p_first, tris.to(dev), t_first, max(p_len))
    d_t = face_point_distance(points.to(dev), p_first, tris.to(dev), t_first, max(p_len))
    want, A = 0.0, 0.0
    for n in range(3):
        d64 = all_pairs(clouds[n], meshes[n])
        p0, t0 = int(p_first[n]), int(t_first[n])
        A_p, A_t = close_both(d_p[p0:p0 + p_len[n]], d_t[t0:t0 + t_len[n]], clouds[n], meshes[n], 0.0, d64)
        want = want + d64.min(dim=1).values.mean() / 3.0 + d64.min(dim=0).values.mean() / 3.0
        A += (A_p + A_t) / 3.0
    # the scalar, from padded inputs: verts / faces with num_faces, a Pointclouds-like object with lengths
    F, P = max(t_len), max(p_len)
    verts = torch.zeros(3, 3 * F, 3)
    faces = torch.zeros(3, F, 3, dtype=torch.int64)
    pad = torch.zeros(3, P, 3)
    for n in range(3):
        verts[n, :3 * t_len[n]] = meshes[n].reshape(-1, 3)
        faces[n, :t_len[n]] = torch.arange(3 * t_len[n]).reshape(-1, 3)
        pad[n, :p_len[n]] = clouds[n]

    class PC(object):
        def points_padded(self):
            return pad.to(dev)

        def num_points_per_cloud(self):
            return torch.tensor(p_len, device=dev)
    got = point_mesh_face_distance((verts.to(dev), faces.to(dev), torch.tensor(t_len)), PC())
    # a mean of values within 1e-5 ref + A each; the float32 sums are trees a dozen additions deep (below 1e-6 relative)
    assert abs(got.item() - want.item()) <= REL * want.item() + A


# ------------------------------------------------------------------------------------------------------ 5. gradients
def tol_grads(points, tris, idx, w, direction):
    g32 = grads_at(points, tris, idx, w, direction, 0.0, torch.float32)
    g64 = grads_at(points, tris, idx, w, direction, 0.0, torch.float64)
    return g64, [4.0 * (a.double() - b).abs().max().item() for a, b in zip(g32, g64)]


@pytest.mark.parametrize("direction", [0, 1])
def test_gradients_against_float64_autograd(dev, direction):
    """Points and triangles, either direction, with a weight per query: against float64 autograd of the oracle at the
    selected pairs."""
    from iso_points_amd import loss
    points, tris = shell_cloud(1500, 21), sphere_tris(2, shrink=0.9)
    p = points.to(dev).requires_grad_(True)
    t = tris.to(dev).requires_grad_(True)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    fn = loss.point_face_distance if direction == 0 else loss.face_point_distance
    d2 = fn(p, first, t, first, 1500)
    w = torch.rand(d2.shape[0], generator=torch.Generator().manual_seed(22)) + 0.5
    (d2 * w.to(dev)).sum().backward()
    pts, tr, seg = loss._pf_inputs(points.to(dev), first, tris.to(dev), first, None, 0.0, "test")
    _, idx, _ = loss._pf_search(direction, pts, tr, seg, 0.0)
    (gp, gt), (A_p, A_t) = tol_grads(points, tris, idx.long(), w, direction)
    print("direction %d: A points %.3g, tris %.3g" % (direction, A_p, A_t))
    close(p.grad, gp, A_p)
    close(t.grad, gt, A_t)


def test_gradient_of_a_face_chosen_by_more_than_a_thousand_points(dev):
    """1500 points against the 20 faces of an icosahedron, 1100 of them above one face: that face's list is longer than
    the 1024 entries a wave sorts, others run through the sorted and the per-lane paths."""
    from iso_points_amd import loss
    tris = sphere_tris(0)
    g = torch.Generator().manual_seed(23)
    c = tris[7].mean(dim=0)
    near = c * 1.2 + (torch.rand(1100, 3, generator=g) - 0.5) * 0.2
    points = torch.cat([shell_cloud(400, 24) * 1.3, near])[torch.randperm(1500, generator=g)]
    p = points.to(dev).requires_grad_(True)
    t = tris.to(dev).requires_grad_(True)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    d2 = loss.point_face_distance(p, first, t, first, 1500)
    w = torch.rand(1500, generator=g) + 0.5
    (d2 * w.to(dev)).sum().backward()
    _, idx = loss.nearest_faces(points.to(dev), tris.to(dev))
    counts = torch.bincount(idx.cpu(), minlength=20)
    assert counts.max() > 1024 and ((counts > 8) & (counts <= 1024)).any(), counts
    (gp, gt), (A_p, A_t) = tol_grads(points, tris, idx, w, 0)
    close(p.grad, gp, A_p)
    close(t.grad, gt, A_t)
    # the mirror: one point chosen by every face
    lone = torch.tensor([[0.1, 0.2, 0.3]]).to(dev).requires_grad_(True)
    fine = sphere_tris(3).to(dev).requires_grad_(True)
    d2 = loss.face_point_distance(lone, first, fine, first, 1)
    d2.sum().backward()
    i_t = torch.zeros(1280, dtype=torch.int64)
    (gp, gt), (A_p, A_t) = tol_grads(lone.detach().cpu(), fine.detach().cpu(), i_t, torch.ones(1280), 1)
    close(lone.grad, gp, A_p)
    close(fine.grad, gt, A_t)


def test_gradient_of_a_long_list_in_the_second_mesh_of_a_packed_batch(dev):
    """Two icosahedra packed, 400 shell points around the first; 1100 points above one face of the second (plus 200 on its
    shell): the list longer than 1024 belongs to a packed face index >= 20 and its queries start at packed row 400.  Point ->
    face with a weight per query."""
    from iso_points_amd import loss
    centre = torch.tensor([4.0, 0.0, 0.0])
    meshes = [sphere_tris(0), sphere_tris(0, centre=(4.0, 0.0, 0.0))]
    g = torch.Generator().manual_seed(27)
    c = meshes[1][7].mean(dim=0) - centre
    near = centre + c * 1.2 + (torch.rand(1100, 3, generator=g) - 0.5) * 0.2
    clouds = [shell_cloud(400, 28) * 1.3,
              torch.cat([shell_cloud(200, 29) * 1.3 + centre, near])[torch.randperm(1300, generator=g)]]
    counts = torch.bincount(all_pairs(clouds[1], meshes[1]).argmin(dim=1), minlength=20)
    assert counts.max() > 1024 and ((counts > 8) & (counts <= 1024)).any(), counts
    points, tris = torch.cat(clouds), torch.cat(meshes)
    p_first, t_first = torch.tensor([0, 400], device=dev), torch.tensor([0, 20], device=dev)
    p = points.to(dev).requires_grad_(True)
    t = tris.to(dev).requires_grad_(True)
    d2 = loss.point_face_distance(p, p_first, t, t_first, 1300)
    w = torch.rand(1700, generator=g) + 0.5
    (d2 * w.to(dev)).sum().backward()
    pts, tr, seg = loss._pf_inputs(points.to(dev), p_first, tris.to(dev), t_first, None, 0.0, "test")
    _, idx, _ = loss._pf_search(0, pts, tr, seg, 0.0)
    # the search's own counts (float32: points nearest to an edge two faces share may go to either face, so they are not
    # the float64 counts to the last point): the list beyond 1024 is the one of that face, behind mesh 0's rows
    packed = torch.bincount(idx.long().cpu(), minlength=40)
    assert packed[:20].max() <= 1024 and int(packed.argmax()) == 20 + int(counts.argmax()) and packed.max() > 1024, packed
    (gp, gt), (A_p, A_t) = tol_grads(points, tris, idx.long(), w, 0)
    print("A points %.3g, tris %.3g" % (A_p, A_t))
    close(p.grad, gp, A_p)
    close(t.grad, gt, A_t)


def test_only_the_requested_gradients_are_computed(dev, monkeypatch):
    from iso_points_amd import _lib, loss
    points, tris = shell_cloud(300, 25), sphere_tris(1)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    seen = []
    real = _lib.call

    def spy(name, *args):
        if name == "iso_pfdist_backward":
            seen.append((args[0], args[6] is not None, args[7] is not None))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    p = points.to(dev).requires_grad_(True)
    loss.point_face_distance(p, first, tris.to(dev), first, 300).sum().backward()
    t = tris.to(dev).requires_grad_(True)
    loss.face_point_distance(points.to(dev), first, t, first, 300).sum().backward()
    verts, faces = icosphere(1)
    v = verts[None].to(dev).requires_grad_(True)
    loss.point_mesh_face_distance((v, faces[None].to(dev)), points[None].to(dev)).backward()
    assert seen[:2] == [(0, True, False), (1, False, True)] and sorted(seen[2:]) == [(0, False, True), (1, False, True)], seen
    assert p.grad is not None and t.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------ 6. determinism, no host read
def run_all(dev, points, verts, faces):
    from iso_points_amd.loss import point_mesh_face_distance
    p = points.to(dev).requires_grad_(True)
    v = verts.to(dev).requires_grad_(True)
    value = point_mesh_face_distance((v, faces.to(dev)), p)
    value.backward()
    return value.detach().clone(), p.grad.clone(), v.grad.clone()


def test_forward_and_backward_are_bit_identical(dev):
    """Twice on the current stream and once on a second stream: the same bits."""
    verts, faces = icosphere(2)
    # every face with vertices of its own: the gradient of verts[faces] is then torch's scatter without collisions, and
    # what is compared is the triangles' gradient as the kernels wrote it
    verts = torch.stack([verts[faces].reshape(-1, 3), verts[faces].reshape(-1, 3) * 0.7])
    faces = torch.arange(verts.shape[1]).reshape(-1, 3)
    faces = torch.stack([faces, faces])
    points = torch.stack([shell_cloud(1200, 26), cube_cloud(1200, 27, half=1.0)])
    first = run_all(dev, points, verts, faces)
    second = run_all(dev, points, verts, faces)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        third = run_all(dev, points, verts, faces)
    stream.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    # and the value is the oracle's
    want, A = 0.0, 0.0
    for n in range(2):
        d64 = all_pairs(points[n], verts[n][faces[n]])
        want = want + d64.min(dim=1).values.mean() / 2.0 + d64.min(dim=0).values.mean() / 2.0
        A += sum(tol_values(points[n], verts[n][faces[n]], 0.0, d64)) / 2.0
    assert abs(first[0].item() - want.item()) <= REL * want.item() + A


def test_default_lengths_read_nothing_back(dev):
    """No device-to-host read in a call whose lengths follow from the shapes: the call can be enqueued behind running
    work."""
    from iso_points_amd.loss import point_mesh_face_distance
    verts, faces = icosphere(2)
    v = verts[None].to(dev).requires_grad_(True)
    f = faces[None].to(dev)
    p = shell_cloud(700, 28)[None].to(dev).requires_grad_(True)
    point_mesh_face_distance((v, f), p).backward()                       # warm: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p.grad = None
        point_mesh_face_distance((v, f), p).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all()
