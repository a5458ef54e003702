"""iso_points_amd.ops.marching_tetrahedra and what is built on it, on the GPU, against the numpy restatement of
tests/mesh_extract_oracle.py (checked on its own in tests/test_mesh_extract_cpu.py; the rule is include/isopoints.h
section N).  Vertices are compared bit for bit and faces as arrays; topology, orientation and area are then computed from
the GPU's arrays alone.

Figures measured on the CPU when the tests were written, float64 restatement:
  * sphere r = 0.6 on 33^3 over [-1, 1]^3: area / (4 pi r^2) - 1 = -2.784e-03.  The assertion allows twice that.
  * get_surface_high_res_mesh's chain on the analytic sphere r = 0.6 at resolution 48 (64^3 mesh -> 10 000 samples -> PCA
    -> aligned grid -> extraction -> rotated back), 10 000 samples of the result against 10 000 points on the exact
    sphere: Chamfer distance (both directions, mean of squared distances) CHAIN_CHAMFER_F64 below -- the distance between
    two samplings of one surface at this density; the mesh's own error is below it.  The assertion allows
    twice that.
"""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_extract_oracle as M

pytestmark = pytest.mark.gpu

SPHERE_AREA_ERR_F64 = 2.784e-3
CHAIN_CHAMFER_F64 = 2.865e-4   # three samplings: 2.832e-04, 2.885e-04, 2.880e-04; two samplings of the exact sphere: 2.880e-04


def _ragged():
    shape, org, spc = (5, 9, 70), (-0.6, -0.4, -0.7), (0.3, 0.1, 0.02)
    return M.volume(lambda p: M.sphere_sdf(p, 0.35), shape, org, spc), org, spc, 0.0


def _boxed(sdf, n, side=2.0, level=0.0):
    shape, org, spc = M.box_grid(n, side)
    return M.volume(sdf, shape, org, spc), org, spc, level


def _minimum():
    vol = np.array([[[-1.0, 0.5], [0.25, 2.0]], [[1.0, -0.125], [3.0, 0.75]]], dtype=np.float32)
    return vol, (0.5, -1.0, 2.0), (1.0, 0.5, 0.25), 0.0


def _on_level():
    shape, org, spc = (9, 4, 5), (-1.0, 0.0, 0.0), (0.25, 0.25, 0.25)
    return M.volume(lambda p: p[..., 0] - 0.25, shape, org, spc), org, spc, 0.0


def _nan_plane():
    vol, org, spc, level = _boxed(lambda p: M.sphere_sdf(p, 0.6), 20)
    vol[:, 9, :] = np.nan
    vol[4, :, 3] = -np.inf
    vol[15, 2, :] = np.inf
    return vol, org, spc, level


CASES = {
    "sphere33": lambda: _boxed(lambda p: M.sphere_sdf(p, 0.6), 33),
    "torus40": lambda: _boxed(lambda p: M.torus_sdf(p, 0.5, 0.2), 40),
    "two_spheres": lambda: _boxed(M.two_spheres_sdf, 36, 2.2),
    "ragged": _ragged,
    "minimum": _minimum,
    "level01": lambda: _boxed(lambda p: M.sphere_sdf(p, 0.5), 24, 2.0, 0.1),
    "cut_sphere": lambda: _boxed(lambda p: M.sphere_sdf(p, 1.2), 21),
    "on_level": _on_level,
    "nan_plane": _nan_plane,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(volume, origin, spacing, level, oracle verts float32, oracle faces): computed once, shared, never written to"""
    vol, org, spc, level = CASES[name]()
    verts, faces = M.extract(vol, org, spc, level)
    for a in (vol, verts, faces):
        a.setflags(write=False)
    return vol, org, spc, level, verts, faces


@functools.lru_cache(maxsize=None)
def gpu_mesh(name):
    from iso_points_amd.ops import marching_tetrahedra
    vol, org, spc, level = case(name)[:4]
    verts, faces = marching_tetrahedra(torch.tensor(vol, device="cuda:0"), org, spc, level)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64 and verts.shape[1:] == (3,) and faces.shape[1:] == (3,)
    return verts.cpu().numpy(), faces.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_equal_to_the_restatement_element_for_element(dev, name):
    _vol, _org, _spc, _level, want_v, want_f = case(name)
    got_v, got_f = gpu_mesh(name)
    print("%s: %d vertices, %d faces" % (name, len(want_v), len(want_f)))
    assert got_v.shape == want_v.shape and got_f.shape == want_f.shape
    assert np.array_equal(got_f, want_f)
    assert np.array_equal(got_v.view(np.int32), want_v.view(np.int32))          # bits, not values
    assert len(want_f) > 0 and not np.isnan(got_v).any()


@pytest.mark.parametrize("name,chi,parts", [("sphere33", 2, 1), ("torus40", 0, 1), ("two_spheres", 4, 2), ("ragged", 2, 1),
                                            ("level01", 2, 1)])
def test_topology_from_the_faces_alone(dev, name, chi, parts):
    from iso_points_amd.ops import mesh_components
    verts, faces = gpu_mesh(name)
    census = M.edge_census(faces)
    assert all(c == [1, 1] for c in census.values())           # every edge in two faces, once in each direction
    assert len(np.unique(faces)) - len(census) + len(faces) == chi
    assert sorted(np.unique(faces)) == list(range(len(verts)))
    labels, areas = mesh_components(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev))
    assert labels.dtype == torch.int64 and areas.dtype == torch.float64 and areas.shape == (parts,)
    assert np.array_equal(labels.cpu().numpy(), M.components(faces))
    _n, area = M.face_normals_areas(verts, faces)
    want = np.array([area[M.components(faces) == c].sum() for c in range(parts)])
    # two float64 sums of ~10^4 terms in different orders: n * 2^-53 ~ 1e-12 relative each
    assert np.abs(areas.cpu().numpy() - want).max() <= 1e-11 * want.max()


def test_largest_component_keeps_the_larger_sphere(dev):
    from iso_points_amd.ops import largest_component, mesh_components
    verts, faces = gpu_mesh("two_spheres")
    v, f = largest_component(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev))
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert 0 < len(f) < len(faces) and sorted(np.unique(f)) == list(range(len(v)))     # re-indexed, nothing unused
    assert M.is_closed_and_oriented(f) and M.euler_characteristic(f) == 2
    r = np.linalg.norm(v.astype(np.float64) - np.array([-0.4, 0.0, 0.0]), axis=1)
    assert np.abs(r - 0.45).max() < 0.01                                               # the sphere of radius 0.45
    lab = M.components(faces)
    big = int(np.argmax([M.face_normals_areas(verts, faces[lab == c])[1].sum() for c in (0, 1)]))
    assert np.array_equal(verts[faces[lab == big]], v[f])                              # the same triangles, in order
    empty_v, empty_f = largest_component(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev))
    assert empty_v.shape == (0, 3) and empty_f.shape == (0, 3)
    assert mesh_components(empty_v, empty_f)[1].shape == (0,)


def test_a_surface_cut_by_the_box_is_open_on_the_box_only(dev):
    verts, faces = gpu_mesh("cut_sphere")
    census = M.edge_census(faces)
    open_edges = [e for e, c in census.items() if c != [1, 1]]
    assert len(open_edges) > 20
    for a, b in open_edges:
        assert sorted(census[(a, b)]) == [0, 1]                                        # a single face
        on_a, on_b = np.abs(np.abs(verts[a]) - 1.0) < 1e-6, np.abs(np.abs(verts[b]) - 1.0) < 1e-6
        assert (on_a & on_b).any()                                                     # both ends on one box face


@pytest.mark.parametrize("name", ["sphere33", "torus40", "two_spheres"])
def test_normals_point_outwards(dev, name):
    verts, faces = gpu_mesh(name)
    n, area = M.face_normals_areas(verts, faces)
    cen = verts[faces].astype(np.float64).mean(1)
    if name == "sphere33":
        grad = cen
    elif name == "torus40":
        grad = M.torus_grad(cen, 0.5, 0.2)
    else:
        c0, c1 = np.array([-0.4, 0.0, 0.0]), np.array([0.55, 0.1, 0.0])
        near0 = M.sphere_sdf(cen, 0.45, c0) < M.sphere_sdf(cen, 0.3, c1)
        grad = np.where(near0[:, None], cen - c0, cen - c1)
    keep = area > 0
    assert keep.sum() > 1000 and ((n[keep] * grad[keep]).sum(1) > 0).all()


@pytest.mark.parametrize("name", ["sphere33", "torus40"])
def test_vertices_lie_on_the_surface(dev, name):
    """The bound is the linear interpolant's own error for this field and spacing: the largest |sdf| over the float64
    restatement's vertices.  The float32 arithmetic adds at most three roundings of half an ulp of 1 per coordinate
    (t, the product, the sum): sqrt(3) * 1.5 * 2^-24 * 2 < 4e-7 in distance, and a distance field is 1-Lipschitz."""
    vol, org, spc, level = case(name)[:4]
    sdf = (lambda p: M.sphere_sdf(p, 0.6)) if name == "sphere33" else (lambda p: M.torus_sdf(p, 0.5, 0.2))
    v64, _f = M.extract(vol, org, spc, level, dtype=np.float64)
    bound = np.abs(sdf(v64)).max()
    got = np.abs(sdf(gpu_mesh(name)[0])).max()
    print("%s: largest |sdf| at a vertex %.3e, float64 restatement %.3e" % (name, got, bound))
    assert got <= bound + 4e-7


def test_area_of_the_sphere(dev):
    vol, org, spc, level = case("sphere33")[:4]
    v64, f64 = M.extract(vol, org, spc, level, dtype=np.float64)
    want = M.face_normals_areas(v64, f64)[1].sum()
    got = M.face_normals_areas(*gpu_mesh("sphere33"))[1].sum()
    exact = 4 * math.pi * 0.6 ** 2
    print("area: GPU %.9f, float64 restatement %.9f, sphere %.9f (%.3e)" % (got, want, exact, got / exact - 1))
    assert abs(got / want - 1) <= 1e-5
    assert abs(got / exact - 1) <= 2 * SPHERE_AREA_ERR_F64


def test_values_on_the_level(dev):
    vol = case("on_level")[0]
    assert (vol[5] == 0).all()
    verts, faces = gpu_mesh("on_level")
    assert not np.isnan(verts).any() and (verts[:, 0] == 0.25).all()
    area = M.face_normals_areas(verts, faces)[1]
    assert (area == 0).any() and (area > 0).any()                                     # kept, not filtered
    assert abs(area.sum() - 0.75) < 1e-6


def test_empty_volumes(dev):
    from iso_points_amd.ops import marching_tetrahedra
    for sign in (1.0, -1.0):
        v, f = marching_tetrahedra(torch.full((7, 3, 66), sign, device=dev))
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64
    v, f = marching_tetrahedra(torch.full((4, 4, 4), float("nan"), device=dev))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    torch.cuda.synchronize()


def test_two_runs_and_a_side_stream_give_the_same_bits(dev):
    from iso_points_amd.ops import marching_tetrahedra
    vol, org, spc, level = case("torus40")[:4]
    x = torch.tensor(vol, device=dev)
    first = marching_tetrahedra(x, org, spc, level)
    second = marching_tetrahedra(x, org, spc, level)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = marching_tetrahedra(x, org, spc, level)
    side.synchronize()
    for other in (second, third):
        assert torch.equal(first[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(first[1], other[1])
    assert np.array_equal(first[1].cpu().numpy(), case("torus40")[5])


def test_refusals_through_the_abi(dev):
    from iso_points_amd import _lib
    from iso_points_amd.ops import marching_tetrahedra
    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    n = 6
    vol = torch.from_numpy(M.volume(lambda p: M.sphere_sdf(p, 0.6), *M.box_grid(n))).to(dev)
    ws_bytes = lib.iso_meshextract_workspace_bytes(n, n, n)
    assert ws_bytes > 17 * n ** 3 and ws_bytes % 16 == 0
    assert lib.iso_meshextract_workspace_bytes(1, n, n) == 0 and lib.iso_meshextract_workspace_bytes(n, 1025, n) == 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    totals = torch.zeros((2,), dtype=torch.int64, device=dev)
    p, s = _lib.ptr, _lib.stream()

    def count(values=vol, dims=(n, n, n), iso=0.0, tot=totals, work=ws, nbytes=ws_bytes):
        return lib.iso_meshextract_count(p(values), dims[0], dims[1], dims[2], iso, p(tot), p(work), nbytes, s)
    for dims in ((1, n, n), (n, 1, n), (n, n, 1), (0, n, n), (-3, n, n)):
        assert count(dims=dims) == INVALID, dims
    for dims in ((1025, n, n), (n, 1025, n), (n, n, 1025)):
        assert count(dims=dims) == UNSUPPORTED, dims
    assert count(values=None) == INVALID and count(tot=None) == INVALID and count(work=None) == INVALID
    assert count(iso=float("nan")) == INVALID
    assert count(nbytes=ws_bytes - 16) == WORKSPACE
    assert b"iso_meshextract_count" in lib.iso_last_error()
    assert count() == 0
    V, F = totals.tolist()
    want_v, want_f = M.extract(vol.cpu().numpy(), *M.box_grid(n)[1:])
    assert (V, F) == (len(want_v), len(want_f)) and V > 0 and F > 0
    verts = torch.full((V + 1, 3), -7.0, device=dev)
    faces = torch.full((F + 1, 3), -7, dtype=torch.int32, device=dev)
    org, spc = M.box_grid(n)[1:]

    def emit(values=vol, dims=(n, n, n), spacing=spc, tot=totals, v=verts, vcap=V, f=faces, fcap=F, work=ws, nbytes=ws_bytes):
        return lib.iso_meshextract_emit(p(values), dims[0], dims[1], dims[2], org[0], org[1], org[2], spacing[0], spacing[1],
                                         spacing[2], 0.0, p(tot), p(v), vcap, p(f), fcap, p(work), nbytes, s)
    assert emit(vcap=V - 1) == INVALID and emit(fcap=F - 1) == INVALID and emit(vcap=0, fcap=0) == INVALID
    assert emit(vcap=-1) == INVALID
    assert emit(dims=(1, n, n)) == INVALID and emit(dims=(n, n, 1025)) == UNSUPPORTED
    assert emit(values=None) == INVALID and emit(tot=None) == INVALID and emit(work=None) == INVALID
    assert emit(v=None) == INVALID and emit(f=None) == INVALID
    assert emit(spacing=(0.0, 0.4, 0.4)) == INVALID and emit(spacing=(0.4, -0.4, 0.4)) == INVALID
    assert emit(nbytes=ws_bytes - 16) == WORKSPACE
    torch.cuda.synchronize()
    assert (verts == -7.0).all() and (faces == -7).all()                             # a refused call writes nothing
    assert emit() == 0
    torch.cuda.synchronize()
    assert np.array_equal(verts[:V].cpu().numpy().view(np.int32), want_v.view(np.int32))
    assert np.array_equal(faces[:F].cpu().numpy(), want_f)
    assert (verts[V:] == -7.0).all() and (faces[F:] == -7).all()                     # nothing beyond the totals
    # the package: no CPU path, and shapes are checked before anything is launched
    with pytest.raises(RuntimeError, match="no CPU path"):
        marching_tetrahedra(torch.zeros(4, 4, 4))
    for bad in (torch.zeros(4, 4, device=dev), torch.zeros(1, 4, 4, device=dev), torch.zeros(2, 2, 1025, device=dev)):
        with pytest.raises(ValueError):
            marching_tetrahedra(bad)
    with pytest.raises(ValueError):
        marching_tetrahedra(vol, spacing=(1.0, 0.0, 1.0))


def test_sdf_grid_on_a_small_siren(dev):
    """sdf_grid runs a SIREN on the fused value-only kernel: the same bits as siren_sdf_and_grad(need_grad=False) on the
    same points.  The volume that torch's own forward gives differs in the last bits but, for this seed, not in any
    inside flag (asserted), and then the two meshes have the same faces and every vertex on the same grid edge."""
    from iso_points_amd.ops import marching_tetrahedra, sdf_grid
    from iso_points_amd.sdf_models import FusedSdf, Siren, siren_sdf_and_grad
    torch.manual_seed(5)
    model = Siren(hidden_size=64, n_layers=2).to(dev)
    n = 17
    axis = torch.from_numpy((np.linspace(-0.5, 0.5, n) * 2.0).astype(np.float32)).to(dev)
    pts = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1)
    with torch.no_grad():                                  # an untrained SIREN: put its mean level at zero
        model.net[-1].bias -= model(pts.reshape(-1, 3)).sdf.mean()
    values, origin, spacing = sdf_grid(model, n, box_side_length=2.0)
    assert values.shape == (n, n, n) and values.dtype == torch.float32
    assert origin == (-1.0, -1.0, -1.0) and spacing == (0.125, 0.125, 0.125)
    direct = siren_sdf_and_grad(model, pts, need_grad=False)[0]
    assert torch.equal(values.view(torch.int32), direct.view(torch.int32))
    assert torch.equal(sdf_grid(FusedSdf(model, dev), n)[0], values)
    assert torch.equal(sdf_grid(model, None, points=pts)[0], values) and sdf_grid(model, None, points=pts)[1] is None
    with torch.no_grad():
        eager = model(pts.reshape(-1, 3)).sdf.reshape(n, n, n)
        chunked = sdf_grid(lambda x: model(x).sdf, None, points=pts)[0]         # any other callable: torch, in chunks
    assert torch.equal(chunked, eager)
    assert (values - eager).abs().max().item() < 1e-4
    assert torch.equal(values < 0, eager < 0), "the two evaluations disagree on an inside flag for this seed"
    va, fa = marching_tetrahedra(values, origin, spacing)
    vb, fb = marching_tetrahedra(eager, origin, spacing)
    print("siren 64 x 2 on 17^3: %d vertices, %d faces" % (va.shape[0], fa.shape[0]))
    assert fa.shape[0] > 100 and torch.equal(fa, fb) and va.shape == vb.shape
    assert (va - vb).abs().max().item() <= 0.125                                  # on the same edge or diagonal
    want_v, want_f = M.extract(values.cpu().numpy(), origin, spacing)
    assert np.array_equal(fa.cpu().numpy(), want_f) and np.array_equal(va.cpu().numpy().view(np.int32), want_v.view(np.int32))


def test_end_to_end_on_the_analytic_sphere(dev):
    """get_surface_high_res_mesh(SphereSDF, 48) -> sample_points_from_meshes -> chamfer_distance against points on the
    exact sphere, within twice what the float64 restatement reaches through the same chain on the CPU."""
    from iso_points_amd.loss import chamfer_distance
    from iso_points_amd.ops import get_surface_high_res_mesh, sample_points_from_meshes
    from iso_points_amd.sdf_models import SphereSDF
    radius = 0.6
    sdf = SphereSDF(radius=radius).to(dev)
    gen = torch.Generator().manual_seed(11)
    verts, faces, normals = get_surface_high_res_mesh(sdf, resolution=48, return_normals=True, generator=gen)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64 and verts.is_cuda and faces.is_cuda
    f = faces.cpu().numpy()
    assert len(f) > 5000 and M.is_closed_and_oriented(f) and M.euler_characteristic(f) == 2
    unit = verts / verts.norm(dim=1, keepdim=True)
    assert (normals.norm(dim=1) - 1).abs().max().item() < 1e-5
    assert ((normals * unit).sum(1) > 0.999).all()                                    # unit and outward
    n_face = M.face_normals_areas(verts.cpu().numpy(), f)[0]
    cen = verts.cpu().numpy()[f].mean(1)
    assert ((n_face * cen).sum(1) > 0).all()                                          # the rotation kept the orientation
    cloud = sample_points_from_meshes((verts[None], faces[None]), 10000, generator=gen)
    g = torch.Generator().manual_seed(12)
    exact = torch.nn.functional.normalize(torch.randn(1, 10000, 3, generator=g), dim=-1).to(dev) * radius
    cham = chamfer_distance(cloud, exact)[0].item()
    print("chamfer distance of the extracted sphere: %.4e (float64 restatement's chain: %.4e)" % (cham, CHAIN_CHAMFER_F64))
    assert cham <= 2 * CHAIN_CHAMFER_F64
    # without the second output, and without a sign change
    v2, f2 = get_surface_high_res_mesh(sdf, resolution=48, generator=torch.Generator().manual_seed(11))
    assert torch.equal(v2, verts) and torch.equal(f2, faces)
    nothing = get_surface_high_res_mesh(SphereSDF(radius=5.0).to(dev), resolution=16, return_normals=True)
    assert [tuple(t.shape) for t in nothing] == [(0, 3)] * 3
