"""iso_points_amd.loss.mesh_pseudonormals / point_mesh_sign / point_mesh_signed_distance on the GPU against the float64
oracle of tests/pfsign_oracle.py (brute force over all pairs, the same pseudonormal rule; the oracle itself is checked
against the generalised winding number in tests/test_pfsign_cpu.py).

Signs are compared exactly on every point whose float64 distance to the mesh exceeds 1e-4 (at most 1 % of a point set may
lie closer; here 0 of 6128 on the torus, 1 of 6008 on the cube).  Nearest faces and feature codes are compared where the
float64 best and second best face differ by more than 1e-5 relative: faces that share an edge or a vertex tie exactly.

Bound for a vector or a gradient entry: |got - ref| <= A, nothing relative.  A is not chosen and never comes from the
kernel: the same formula runs in torch float32 on the CPU on the inputs of the test at hand, and A is 4 x its largest error
against float64.  One floor, from the number format: no float32 result can be expected nearer to the reference than half a
float32 step at the largest reference entry (a sum added in another order lands a whole step away), so where the CPU
evaluation happens to land nearer than that (a fan of 9: 7.5e-08 on a sum of 4.94, whose step is 4.8e-07), half a step
stands in for the measured error: A >= 2 steps.  Measured on the CPU (largest float32 error -> A):
    pseudonormals  torus 16 x 8   face 9.0e-08 -> 3.6e-07   edge 2.1e-07 -> 8.2e-07   vertex 5.6e-07 -> 2.2e-06
                   fan of 40      face 5.2e-08 -> 2.1e-07   edge 1.0e-07 -> 4.2e-07   vertex 1.4e-06 -> 5.4e-06
                   fan of 1100    face 1.8e-06 -> 7.0e-06   edge 2.8e-06 -> 1.1e-05   vertex 3.9e-05 -> 1.5e-04
                   (the fan's faces are slivers of 0.33 degrees at the apex: their cross product cancels)
    signed distance, torus        value 2.1e-07 -> 8.4e-07  grad points 8.5e-05 -> 3.4e-04  grad verts 7.2e-05 -> 2.9e-04
                   (the gradient's float32 formula is the backward pass as documented, 2 r with the closest point held:
                   signed_distance_f32; the nearest of the 2500 points is 4e-4 from the surface, where r / |r| feels
                   the rounding of p - c)"""
import math

import pytest
import torch

import pfsign_oracle as O

pytestmark = pytest.mark.gpu

NEAR = 1e-4


def mesh_of(dev, verts, faces):
    return verts[None].to(dev), faces[None].to(dev)


def sign_parts(dev, verts, faces, points, **kw):
    from iso_points_amd.loss import point_mesh_sign
    sign, idx, feature = point_mesh_sign(mesh_of(dev, verts, faces), points.to(dev), return_parts=True, **kw)
    assert sign.dtype == torch.float32 and idx.dtype == torch.int64 and feature.dtype == torch.int32
    assert sign.shape == idx.shape == feature.shape == (points.shape[0],)
    return sign.cpu(), idx.cpu(), feature.cpu()


def tolerance(f32, ref):
    """A: 4 x the largest error of the float32 CPU evaluation f32 against the float64 reference ref, the error taken as at
    least half a float32 step at the largest reference entry."""
    err = (f32.double() - ref.double()).abs().max().item() if ref.numel() else 0.0
    top = ref.abs().max().item() if ref.numel() else 0.0
    half_step = 0.5 * 2.0 ** (math.floor(math.log2(top)) - 23) if top > 0 else 0.0
    return 4.0 * max(err, half_step), err


def close(got, ref, A, what=""):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = (got - ref).abs() > A
    assert not bad.any(), "%s: %d of %d beyond %.3g: worst |d| = %.3g" % (
        what, int(bad.sum()), bad.numel(), A, (got - ref).abs().max().item())


def assert_signs(sign, ref, what):
    """Exact signs on every point farther than NEAR from the mesh; at most 1 % of the points may be nearer."""
    far = ref["dist"] > NEAR
    print("%s: %d of %d points within %.0e of the mesh, min distance %.3g" % (
        what, int((~far).sum()), far.numel(), NEAR, ref["dist"].min().item()))
    assert (~far).float().mean().item() <= 0.01
    assert set(sign.unique().tolist()) <= {-1.0, 1.0}
    wrong = (sign.double() != ref["sign"]) & far
    assert not wrong.any(), "%s: %d wrong signs, e.g. point %d" % (what, int(wrong.sum()), int(torch.nonzero(wrong)[0]))


# ------------------------------------------------------------------------------------------------ 1. the tetrahedron
def tetrahedron_points():
    """(points, robust (P,) bool, outside (P,) bool): along every face normal at +-0.05 and +-0.5 from the face centre;
    beyond every edge midpoint and every vertex by 0.3 along the feature's pseudonormal (robust: well inside the feature's
    region) and along each incident face's normal (on the border between two regions: only the sign is known)."""
    verts, faces = O.tetrahedron()
    fn, en, vn = O.pseudonormals(verts.double(), faces)
    pts, robust, outside = [], [], []
    for f in range(4):
        c = verts[faces[f]].double().mean(dim=0)
        for s in (0.05, -0.05, 0.5, -0.5):
            pts.append(c + s * fn[f]); robust.append(True); outside.append(s > 0)
    for f in range(4):
        for k in range(3):
            a, b = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            mid = 0.5 * (verts[a] + verts[b]).double()
            if a < b:
                pts.append(mid + 0.3 * en[f, k] / en[f, k].norm()); robust.append(True); outside.append(True)
            pts.append(mid + 0.3 * fn[f]); robust.append(False); outside.append(True)
            pts.append(verts[a].double() + 0.3 * fn[f]); robust.append(False); outside.append(True)
    for v in range(4):
        pts.append(verts[v].double() + 0.3 * vn[v] / vn[v].norm()); robust.append(True); outside.append(True)
    return torch.stack(pts).float(), torch.tensor(robust), torch.tensor(outside)


def test_regular_tetrahedron_exact_signs_and_all_seven_features(dev):
    """The case the plain face-normal rule fails: face normals with dot -1/3, so a point beyond an edge along one face's
    normal lies behind the other face."""
    verts, faces = O.tetrahedron()
    points, robust, outside = tetrahedron_points()
    sign, idx, feature = sign_parts(dev, verts, faces, points)
    assert torch.equal(sign, torch.where(outside, 1.0, -1.0)), (sign, outside)
    assert (sign[:16].reshape(4, 4) == torch.tensor([1.0, -1.0, 1.0, -1.0])).all()      # insides negative
    ref = O.signed(points, verts.double(), faces)
    assert torch.equal(sign.double(), ref["sign"])
    # the feature the kernel names on the face it chose is the float64 oracle's for that pair
    want = O.feature_of(O.pair_closest(points.double(), verts.double()[faces[idx]])[1])
    assert torch.equal(feature[robust], want[robust])
    assert set(feature[robust].tolist()) == set(range(7)), feature[robust].tolist()
    assert (idx >= 0).all() and (idx < 4).all()
    # face probes choose their face; vertex probes are ties between three faces: the lowest index
    assert idx[:16].tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    assert idx[-4:].tolist() == [0, 0, 0, 1] and feature[-4:].tolist() == [4, 5, 6, 5]


# ------------------------------------------------------------------------------------------------ 2. torus and cube
@pytest.mark.parametrize("name", ["torus", "cube"])
def test_signs_indices_and_features_against_float64(dev, name):
    verts, faces, points, ref = O.case(name)
    sign, idx, feature = sign_parts(dev, verts, faces, points)
    assert_signs(sign, ref, name)
    ok = ref["clear"]
    print("%s: clear %.3f of the points; features %s" % (name, ok.float().mean().item(),
                                                        torch.bincount(feature.long(), minlength=7).tolist()))
    assert ok.float().mean().item() > 0.5                                  # the comparison below is not an empty one
    assert torch.equal(idx[ok], ref["idx"][ok]) and torch.equal(feature[ok], ref["feature"][ok])
    assert (torch.bincount(feature.long(), minlength=7) > 0).all()
    # on a tie the kernel's feature is still the oracle's feature of the face the kernel chose, wherever that pair's
    # classification is not itself on a border (every weight either exactly zero or above 1e-4)
    w64 = O.pair_closest(points.double(), verts.double()[faces[idx]])[1]
    firm = ((w64 == 0) | (w64 > 1e-4)).all(dim=1)
    assert firm.float().mean().item() > 0.95
    assert torch.equal(feature[firm], O.feature_of(w64)[firm])


# ------------------------------------------------------------------------------------------------ 3. the vectors
def normals_case(name):
    if name == "torus":
        return O.torus(16, 8)
    return O.fan(int(name[3:]))


@pytest.mark.parametrize("name", ["torus", "fan8", "fan9", "fan40", "fan1024", "fan1100"])
def test_pseudonormal_vectors_against_float64(dev, name):
    """The torus (lists of 6 corners: the lane path); fans of 8 / 9 faces round an apex (either side of kLightList), of 40
    (one wave, sorted), of 1024 and of 1100 (either side of kSortList: the scanning wave)."""
    from iso_points_amd.loss import mesh_pseudonormals
    verts, faces = normals_case(name)
    got = mesh_pseudonormals(mesh_of(dev, verts, faces))
    ref = O.pseudonormals(verts.double(), faces)
    f32 = O.pseudonormals(verts, faces)
    assert [tuple(t.shape) for t in got] == [(faces.shape[0], 3), (faces.shape[0], 3, 3), (verts.shape[0], 3)]
    for g, r, s, what in zip(got, ref, f32, ("face", "edge", "vertex")):
        A, err = tolerance(s, r)
        print("%s %s: float32 error %.3g -> A %.3g; kernel error %.3g" % (
            name, what, err, A, (g.cpu().double() - r).abs().max().item()))
        assert g.dtype == torch.float32 and torch.isfinite(g).all()
        close(g, r, A, name + " " + what)
    if name != "torus":
        n = faces.shape[0]
        assert torch.bincount(faces.reshape(-1))[0].item() == n            # the apex's list has n corners
        # an open cone: rim edges are boundary edges and hold their one face's normal
        assert torch.equal(got[1][:, 1].cpu(), got[0].cpu())


# ------------------------------------------------------------------------------------------------ 4. open and odd meshes
def box_points(n, seed, half=1.5):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0) * half


def test_a_single_triangle_and_a_square_are_signed_by_the_side_of_their_plane(dev):
    points = box_points(1500, 41)
    points = points[points[:, 2].abs() > 1e-3]
    tri_v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    sq_v = torch.tensor([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]])
    for verts, faces in ((tri_v, torch.tensor([[0, 1, 2]])), (sq_v, torch.tensor([[0, 1, 2], [0, 2, 3]]))):
        sign, idx, feature = sign_parts(dev, verts, faces, points)
        assert torch.equal(sign, torch.where(points[:, 2] > 0, 1.0, -1.0))
        assert (torch.bincount(feature.long(), minlength=7) > 0).all()
        flipped, _, _ = sign_parts(dev, verts, faces[:, [0, 2, 1]], points)
        assert torch.equal(flipped, -sign)


def test_three_faces_sharing_one_edge(dev):
    """A non-manifold edge gets the normals of all of its faces, in every face's own slot."""
    from iso_points_amd.loss import mesh_pseudonormals
    verts = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-0.5, 0.875, 0.0], [-0.5, -0.875, 0.0]])
    faces = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    fn, en, vn = (t.cpu() for t in mesh_pseudonormals(mesh_of(dev, verts, faces)))
    total = (fn[0] + fn[1]) + fn[2]
    assert torch.equal(en[0, 0], total) and torch.equal(en[1, 0], total) and torch.equal(en[2, 0], total)
    assert torch.equal(en[0, 1], fn[0]) and torch.equal(en[1, 2], fn[1])           # the others are boundary edges
    points = box_points(1500, 42)
    ref = O.signed(points, verts.double(), faces)
    sign, idx, feature = sign_parts(dev, verts, faces, points)
    assert_signs(sign, ref, "three faces on one edge")
    assert ref["clear"].float().mean().item() > 0.5
    assert torch.equal(idx[ref["clear"]], ref["idx"][ref["clear"]])


def test_faces_without_area_change_nothing(dev):
    """Faces with a repeated vertex on real edges of the torus, put FIRST so that they win every tie of distance, and faces
    with three collinear vertices (coordinates with few bits: the normal is exactly zero) outside the points' box: no NaN,
    the same signs, and the vectors of the real faces and vertices as without them."""
    from iso_points_amd.loss import mesh_pseudonormals
    verts, faces, points, ref = O.case("torus")
    plain = sign_parts(dev, verts, faces, points)
    extra_v = torch.tensor([[8.0, 8.0, 8.0], [8.5, 8.25, 8.0], [9.0, 8.5, 8.0]])
    V = verts.shape[0]
    twice = torch.stack([faces[5, [0, 0, 1]], faces[77, [1, 2, 2]], faces[200, [2, 0, 2]]])
    odd_f = torch.cat([twice, faces, torch.tensor([[V, V + 1, V + 2], [V + 2, V, V + 1]])])
    odd_v = torch.cat([verts, extra_v])
    sign, idx, feature = sign_parts(dev, odd_v, odd_f, points)
    assert torch.equal(sign, plain[0])
    assert_signs(sign, ref, "torus with faces without area")
    assert (idx < 3).sum() > 0 and (idx < 3 + faces.shape[0]).all()                  # the repeated-vertex faces win ties
    a = mesh_pseudonormals(mesh_of(dev, verts, faces))
    b = mesh_pseudonormals(mesh_of(dev, odd_v, odd_f))
    for t in b:
        assert torch.isfinite(t).all()
    assert torch.equal(b[0][3:-2], a[0]) and torch.equal(b[1][3:-2], a[1]) and torch.equal(b[2][:V], a[2])
    assert not b[0][:3].any() and not b[0][-2:].any() and not b[2][V:].any() and not b[1][-2:].any()


def test_a_mesh_without_faces(dev):
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign, point_mesh_signed_distance
    mesh = (torch.rand(1, 4, 3).to(dev), torch.zeros(1, 0, 3, dtype=torch.int64, device=dev))
    points = box_points(300, 43).to(dev)
    sign, idx, feature = point_mesh_sign(mesh, points, return_parts=True)
    assert (sign == 1.0).all() and (idx == -1).all() and (feature == -1).all()
    fn, en, vn = mesh_pseudonormals(mesh)
    assert fn.shape == (0, 3) and en.shape == (0, 3, 3) and vn.shape == (4, 3) and not vn.any()
    assert point_mesh_signed_distance(mesh, points).shape == (300,)
    # and no points
    none = point_mesh_sign(mesh_of(dev, *O.tetrahedron()), torch.zeros(0, 3, device=dev))
    assert none.shape == (0,)


def test_reversed_winding_reverses_every_sign(dev):
    verts, faces, points, ref = O.case("torus")
    sign, _, _ = sign_parts(dev, verts, faces, points)
    flipped, _, _ = sign_parts(dev, verts, faces[:, [0, 2, 1]], points)
    assert torch.equal(flipped, -sign) and (sign < 0).sum() > 1000


# ------------------------------------------------------------------------------------------------ 5. batch
class StubMeshes(object):
    """What the loss reads of a pytorch3d Meshes: two meshes of different sizes, packed."""

    def __init__(self, meshes, dev):
        self.m, self.dev = meshes, dev

    def verts_packed(self):
        return torch.cat([v for v, _ in self.m]).to(self.dev)

    def faces_packed(self):
        out, base = [], 0
        for v, f in self.m:
            out.append(f.to(torch.int32) + base)                                      # not int64: the loss casts
            base += v.shape[0]
        return torch.cat(out).to(self.dev)

    def mesh_to_faces_packed_first_idx(self):
        first, acc = [], 0
        for _, f in self.m:
            first.append(acc)
            acc += f.shape[0]
        return torch.tensor(first, device=self.dev)

    def num_faces_per_mesh(self):
        return torch.tensor([f.shape[0] for _, f in self.m], device=self.dev)


def test_batch_of_two_meshes_and_ragged_clouds(dev):
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign
    meshes = [O.tetrahedron(), O.torus(16, 8)]
    clouds = [tetrahedron_points()[0], O.case("torus")[2][:1500]]
    singles = [sign_parts(dev, v, f, c) for (v, f), c in zip(meshes, clouds)]
    lens = [c.shape[0] for c in clouds]
    Vm, Fm, Pm = max(v.shape[0] for v, _ in meshes), max(f.shape[0] for _, f in meshes), max(lens)
    verts, faces, pad = torch.zeros(2, Vm, 3), torch.zeros(2, Fm, 3, dtype=torch.int64), torch.zeros(2, Pm, 3)
    for n, ((v, f), c) in enumerate(zip(meshes, clouds)):
        verts[n, :v.shape[0]], faces[n, :f.shape[0]], pad[n, :lens[n]] = v, f, c

    class PC(object):
        def points_padded(self):
            return pad.to(dev)

        def num_points_per_cloud(self):
            return torch.tensor(lens, device=dev)
    f_off = [0, meshes[0][1].shape[0]]
    want_sign = torch.cat([s[0] for s in singles])
    want_idx = torch.cat([s[1] + o for s, o in zip(singles, f_off)])
    want_feature = torch.cat([s[2] for s in singles])
    tuple_form = (verts.to(dev), faces.to(dev), torch.tensor([f.shape[0] for _, f in meshes]))
    stub = StubMeshes(meshes, dev)
    for mesh in (tuple_form, stub):
        normals = mesh_pseudonormals(mesh)
        for kw in ({}, {"normals": normals}):
            sign, idx, feature = point_mesh_sign(mesh, PC(), return_parts=True, **kw)
            assert torch.equal(sign.cpu(), want_sign) and torch.equal(idx.cpu(), want_idx)
            assert torch.equal(feature.cpu(), want_feature)
    # the packed vectors of the batch are the meshes' own, one after the other
    one = [mesh_pseudonormals(mesh_of(dev, v, f)) for v, f in meshes]
    for k, got in enumerate(mesh_pseudonormals(stub)):
        assert torch.equal(got, torch.cat([one[0][k], one[1][k]]))


# ------------------------------------------------------------------------------------------------ 6. the signed distance
def signed_distance_ref(points, verts, faces, idx, sign):
    """float64: sign * sqrt(clamp(|d2|, 1e-17)) at the fixed nearest faces and its autograd w.r.t. points and verts, for
    the upstream weights w."""
    p = points.detach().cpu().double().requires_grad_(True)
    v = verts.detach().cpu().double().requires_grad_(True)
    d2 = O.pair_closest(p, v[faces][idx])[0]
    value = sign.double() * d2.abs().clamp_min(1e-17).sqrt()
    w = torch.linspace(0.5, 1.5, value.shape[0], dtype=torch.float64)
    (value * w).sum().backward()
    return value.detach(), p.grad, v.grad, w


def signed_distance_f32(points, verts, faces, idx, sign, w):
    """The same in float32 by the formulas the package documents (include/isopoints.h section H): the value from d2, and
    the backward pass with the closest point held: r = p - c, d d2 / d p = 2 r, d d2 / d v_k = -2 b_k r, each times the
    upstream weight of d2, here w * sign / (2 sqrt(d2)).  (Autograd through the weights b(p) would also project r onto the
    face normal, which the kernels do not do: r keeps the rounding of p - c, and near the surface r / |r| feels it.)"""
    p, tri = points.float(), verts.float()[faces][idx]
    d2, bw = O.pair_closest(p, tri)
    root = d2.abs().clamp_min(1e-17).sqrt()
    r = p - ((bw[:, 0:1] * tri[:, 0] + bw[:, 1:2] * tri[:, 1]) + bw[:, 2:3] * tri[:, 2])
    up2 = 2.0 * (w.float() * sign.float() * 0.5 / root)
    g_tri = -(up2[:, None] * bw)[:, :, None] * r[:, None, :]                                   # (P,3,3)
    g_verts = torch.zeros_like(verts, dtype=torch.float32).index_add_(0, faces[idx].reshape(-1), g_tri.reshape(-1, 3))
    return sign.float() * root, up2[:, None] * r, g_verts


def test_signed_distance_values_and_gradients(dev):
    from iso_points_amd.loss import point_mesh_signed_distance, point_mesh_sign
    verts, faces, points, ref = O.case("torus")
    points = points[:2500]
    p = points.to(dev).requires_grad_(True)
    v = verts[None].to(dev).requires_grad_(True)
    value = point_mesh_signed_distance((v, faces[None].to(dev)), p)
    sign, idx, _ = point_mesh_sign((v.detach(), faces[None].to(dev)), points.to(dev), return_parts=True)
    assert value.shape == (2500,) and torch.equal(torch.sign(value.detach()), sign)
    far = ref["dist"][:2500] > NEAR
    assert torch.equal(sign.cpu().double()[far], ref["sign"][:2500][far])
    v64, gp64, gv64, w = signed_distance_ref(points, verts, faces, idx.cpu(), sign.cpu())
    v32, gp32, gv32 = signed_distance_f32(points, verts, faces, idx.cpu(), sign.cpu(), w)
    A = [tolerance(a, b)[0] for a, b in ((v32, v64), (gp32, gp64), (gv32, gv64))]
    print("A: value %.3g, grad points %.3g, grad verts %.3g" % tuple(A))
    close(value, v64, A[0], "value")
    # and against the oracle's own nearest faces: the same distance
    close(value.detach().abs(), ref["dist"][:2500], A[0], "distance")
    (value * w.float().to(dev)).sum().backward()
    close(p.grad, gp64, A[1], "grad points")
    close(v.grad[0], gv64, A[2], "grad verts")


def test_only_the_requested_gradients_are_computed(dev, monkeypatch):
    from iso_points_amd import _lib, loss
    verts, faces, points, _ = O.case("torus")
    seen = []
    real = _lib.call

    def spy(name, *args):
        if name == "iso_pfdist_backward":
            seen.append((args[0], args[6] is not None, args[7] is not None))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    mesh = mesh_of(dev, verts, faces)
    normals = loss.mesh_pseudonormals(mesh)
    p = points[:500].to(dev).requires_grad_(True)
    loss.point_mesh_signed_distance(mesh, p, normals=normals).sum().backward()
    v = verts[None].to(dev).requires_grad_(True)
    loss.point_mesh_signed_distance((v, mesh[1]), points[:500].to(dev)).sum().backward()
    assert seen == [(0, True, False), (0, False, True)], seen
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0
    assert not loss.point_mesh_sign(mesh, p).requires_grad


# ------------------------------------------------------------------------------------------------ 7. determinism
def run_all(dev, verts, faces, points):
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign, point_mesh_signed_distance
    # every face with vertices of its own for the gradient: the step from the triangles to shared vertices would be torch's
    # scatter, whose order is not this package's
    own_v = verts[faces].reshape(1, -1, 3).to(dev).requires_grad_(True)
    own_f = torch.arange(faces.shape[0] * 3, device=dev).reshape(1, -1, 3)
    p = points.to(dev).requires_grad_(True)
    mesh = mesh_of(dev, verts, faces)
    normals = mesh_pseudonormals(mesh)
    sign, idx, feature = point_mesh_sign(mesh, points.to(dev), normals=normals, return_parts=True)
    value = point_mesh_signed_distance((own_v, own_f), p)
    value.sum().backward()
    return [t.clone() for t in normals] + [sign, idx, feature, value.detach().clone(), p.grad.clone(), own_v.grad.clone()]


def test_two_runs_and_a_side_stream_give_the_same_bits(dev):
    verts, faces, points, _ = O.case("torus")
    fan_v, fan_f = O.fan(1100)                                            # the sorted and the scanning wave as well
    first = run_all(dev, verts, faces, points) + run_all(dev, fan_v, fan_f, points[:500])
    second = run_all(dev, verts, faces, points) + run_all(dev, fan_v, fan_f, points[:500])
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        third = run_all(dev, verts, faces, points) + run_all(dev, fan_v, fan_f, points[:500])
    stream.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_default_lengths_read_nothing_back(dev):
    """No device-to-host read in calls whose lengths follow from the shapes."""
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_signed_distance
    verts, faces, points, _ = O.case("torus")
    mesh = mesh_of(dev, verts, faces)
    p = points[:700].to(dev).requires_grad_(True)
    point_mesh_signed_distance(mesh, p).sum().backward()                  # warm: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p.grad = None
        normals = mesh_pseudonormals(mesh)
        point_mesh_signed_distance(mesh, p, normals=normals).sum().backward()
        point_mesh_signed_distance(mesh, p[None]).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(p.grad).all()
