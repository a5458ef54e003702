"""iso_points_amd.ops.marching_tetrahedra_bricks / sparse_level_set on the GPU (include/isopoints.h section O, DESIGN.md
3.4k) against the dense kernels of section N and the numpy restatements tests/mesh_extract_oracle.py and
tests/mesh_sparse_oracle.py (checked on their own in tests/test_mesh_sparse_cpu.py).  Vertices are compared bit for bit and
faces as arrays.

Figure measured on the CPU when the tests were written, float64 restatement (M.extract): sphere r = 0.1 centred on a grid
point of a box of side 2 at 193 points per side (h0 = 2 / 192, r / h0 = 9.6): area / (4 pi r^2) - 1 = -2.784e-03; at 97 per
side -1.119e-02, so the error is second order in h (ratio 4.02).  test_past_the_dense_limit allows
2 * 2.784e-3 * (h / h0)^2 = 8.70e-05 at 1537 per side.
"""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_extract_oracle as M
import mesh_sparse_oracle as S

pytestmark = pytest.mark.gpu

SPHERE01_AREA_ERR_F64, SPHERE01_H0 = 2.784e-3, 2.0 / 192
CHAIN_CHAMFER_F64 = 2.865e-4          # tests/test_mesh_extract_gpu.py: the dense chain's documented value
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
SPLIT_GRID = ((40, 40, 40), (0.15 - 24 * 0.06, -1.17, -1.17), (0.06, 0.06, 0.06))     # tests/test_mesh_sparse_cpu.py


def _boxed(sdf, n, side=2.0, level=0.0):
    shape, org, spc = M.box_grid(n, side)
    return M.volume(sdf, shape, org, spc), org, spc, level


def _ragged():
    shape, org, spc = (20, 27, 35), (-0.9, -1.0, -1.1), (0.1, 0.08, 0.065)
    return M.volume(lambda p: M.sphere_sdf(p, 0.7), shape, org, spc), org, spc, 0.0


def _nan_plane():
    vol, org, spc, level = _boxed(lambda p: M.sphere_sdf(p, 0.6), 20)
    vol[:, 9, :] = np.nan
    vol[4, :, 3] = -np.inf
    vol[15, 2, :] = np.inf
    return vol, org, spc, level


def _on_level():
    shape, org, spc = (9, 4, 5), (-1.0, 0.0, 0.0), (0.25, 0.25, 0.25)
    return M.volume(lambda p: p[..., 0] - 0.25, shape, org, spc), org, spc, 0.0


def _minimum():
    vol = np.array([[[-1.0, 0.5], [0.25, 2.0]], [[1.0, -0.125], [3.0, 0.75]]], dtype=np.float32)
    return vol, (0.5, -1.0, 2.0), (1.0, 0.5, 0.25), 0.0


CASES = {
    "sphere33": lambda: _boxed(lambda p: M.sphere_sdf(p, 0.6), 33),
    "torus40": lambda: _boxed(lambda p: M.torus_sdf(p, 0.5, 0.2), 40),
    "two_spheres": lambda: _boxed(M.two_spheres_sdf, 36, 2.2),
    "ragged": _ragged,                                            # partial bricks on every axis: 20 = 16 + 4, 27 = 24 + 3, 35 = 32 + 3
    "nan_plane": _nan_plane,
    "on_level": _on_level,
    "level01": lambda: _boxed(lambda p: M.sphere_sdf(p, 0.5), 24, 2.0, 0.1),
    "nine": lambda: _boxed(lambda p: M.sphere_sdf(p, 0.7), 9),    # one cell-block, eight point bricks
    "minimum": _minimum,                                          # 2 x 2 x 2
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(volume, origin, spacing, level, oracle verts float32, oracle faces) of the dense rule: computed once, never written to"""
    vol, org, spc, level = CASES[name]()
    verts, faces = M.extract(vol, org, spc, level)
    for a in (vol, verts, faces):
        a.setflags(write=False)
    return vol, org, spc, level, verts, faces


def _bricked(vol, bricks, active, dev):
    coords = torch.tensor(bricks, dtype=torch.int32, device=dev).reshape(-1, 3)
    values = torch.from_numpy(S.to_bricks(vol, bricks)).to(dev)                     # NaN outside the grid: must be ignored
    act = {tuple(b) for b in active}
    flags = torch.tensor([tuple(b) in act for b in bricks], dtype=torch.uint8, device=dev)
    return values, coords, flags


def _sorted_np(verts, faces, vkey, fcell):
    return S.sort_by_keys(verts.cpu().numpy(), faces.cpu().numpy(), vkey.cpu().numpy(), fcell.cpu().numpy())


@pytest.mark.parametrize("name", sorted(CASES))
def test_all_blocks_active_is_the_dense_mesh(dev, name):
    from iso_points_amd.ops import marching_tetrahedra, marching_tetrahedra_bricks
    vol, org, spc, level, want_v, want_f = case(name)
    bricks = S.all_blocks(vol.shape)
    values, coords, flags = _bricked(vol, bricks, bricks, dev)
    v, f, vk, fc, need = marching_tetrahedra_bricks(values, coords, flags, vol.shape, org, spc, level, return_keys=True,
                                                    return_need=True)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and vk.dtype == torch.int64 and fc.dtype == torch.int64
    assert need.dtype == torch.uint8 and need.shape == (len(bricks),) and int(need.max()) == 0
    got_v, got_f = _sorted_np(v, f, vk, fc)
    print("%s: %d bricks, %d vertices, %d faces" % (name, len(bricks), len(want_v), len(want_f)))
    assert len(want_f) > 0 and got_v.shape == want_v.shape and got_f.shape == want_f.shape
    assert np.array_equal(got_f, want_f) and np.array_equal(got_v.view(np.int32), want_v.view(np.int32))
    dense_v, dense_f = marching_tetrahedra(torch.tensor(vol, device=dev), org, spc, level)
    assert np.array_equal(got_f, dense_f.cpu().numpy()) and np.array_equal(got_v.view(np.int32), dense_v.cpu().numpy().view(np.int32))
    # the keys are the dense (point, slot) numbers of the oracle's own order
    sv, sf, svk, sfc = S.restrict(vol, bricks, org, spc, level)
    assert np.array_equal(vk.cpu().numpy(), svk) and np.array_equal(fc.cpu().numpy(), sfc)
    assert np.array_equal(f.cpu().numpy(), sf) and np.array_equal(v.cpu().numpy().view(np.int32), sv.view(np.int32))


def _subsets(name):
    vol = case(name)[0]
    blocks = S.all_blocks(vol.shape)
    rng = np.random.default_rng(7)
    return {"checkerboard": [b for b in blocks if sum(b) % 2 == 0], "odd": [b for b in blocks if sum(b) % 2 == 1],
            "half": [b for b in blocks if rng.random() < 0.5]}


@pytest.mark.parametrize("pick", ["checkerboard", "odd", "half"])
@pytest.mark.parametrize("name", ["sphere33", "ragged", "nan_plane"])
def test_a_subset_of_blocks_is_the_restriction_in_the_sparse_order(dev, name, pick):
    """The list holds the sampled bricks of the subset (b + {0,1}^3), cell-active on the subset only.  Checkerboards put
    active and inactive blocks side by side everywhere, the far faces of the grid (partial bricks, bricks without a cell)
    and the near ones (no lower neighbour) included."""
    from iso_points_amd.ops import marching_tetrahedra_bricks
    vol, org, spc, level = case(name)[:4]
    active = _subsets(name)[pick]
    bricks = S.sampled(active, vol.shape)
    values, coords, flags = _bricked(vol, bricks, active, dev)
    v, f, vk, fc, need = marching_tetrahedra_bricks(values, coords, flags, vol.shape, org, spc, level, return_keys=True,
                                                    return_need=True)
    want_v, want_f, want_vk, want_fc = S.restrict(vol, active, org, spc, level)
    want_need = S.needed(vol, active, level)
    print("%s/%s: %d of %d bricks active, %d vertices, %d faces, %d bricks with a need" %
          (name, pick, len(active), len(bricks), len(want_v), len(want_f), len(want_need)))
    assert len(want_f) > 0 and len(want_need) > 0
    assert np.array_equal(vk.cpu().numpy(), want_vk) and np.array_equal(fc.cpu().numpy(), want_fc)
    assert np.array_equal(f.cpu().numpy(), want_f)
    assert np.array_equal(v.cpu().numpy().view(np.int32), want_v.view(np.int32))
    assert need.cpu().numpy().tolist() == [want_need.get(tuple(b), 0) for b in bricks]
    # the caller's order does not matter: the list is sorted inside, need comes back in the caller's order
    perm = torch.randperm(len(bricks), generator=torch.Generator().manual_seed(1)).to(dev)
    again = marching_tetrahedra_bricks(values[perm], coords[perm], flags[perm], vol.shape, org, spc, level, return_need=True)
    assert torch.equal(again[0].view(torch.int32), v.view(torch.int32)) and torch.equal(again[1], f)
    assert torch.equal(again[2], need[perm])


def _two_spheres_torch(x):
    """min of the two exact distances of M.two_spheres_sdf, every operation elementwise: a point's value does not depend on
    its batch"""
    def ball(cx, cy, cz, r):
        dx, dy, dz = x[:, 0] - cx, x[:, 1] - cy, x[:, 2] - cz
        return torch.sqrt(dx * dx + dy * dy + dz * dz) - r
    return torch.minimum(ball(-0.4, 0.0, 0.0, 0.45), ball(0.55, 0.1, 0.0, 0.3))


def _axes(shape, org, spc, dev):
    return [torch.from_numpy(a).to(dev) for a in M.grid_axes(shape, org, spc)]


def _closed_oriented_chi(faces):
    """(closed and consistently oriented, Euler characteristic) from the faces alone, vectorised"""
    f = np.asarray(faces, dtype=np.int64)
    n = int(f.max()) + 1
    u = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    v = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    fwd, back = np.sort(u * n + v), np.sort(v * n + u)
    ok = len(np.unique(fwd)) == len(fwd) and np.array_equal(fwd, back)       # every directed edge once, and its reverse
    return ok, len(np.unique(f)) - len(fwd) // 2 + len(f)


def test_closure_follows_one_component_and_band_seeding_finds_all(dev):
    from iso_points_amd.ops import marching_tetrahedra, sparse_level_set
    shape, org, spc = SPLIT_GRID
    axes = _axes(shape, org, spc, dev)
    seed = torch.tensor([[-0.85, 0.0, 0.0]], device=dev)                      # the first sphere's far pole
    v, f, info = sparse_level_set(_two_spheres_torch, shape, org, spc, axes=axes, band=0, seeds=seed, return_info=True)
    print("one seed: %r" % (info,))
    assert info["rounds"] > 1 and info["seed_blocks"] == 1 and info["cell_active_bricks"] > 1
    assert info["points_evaluated"] == 512 * info["sampled_bricks"] < 40 ** 3
    ok, chi = _closed_oriented_chi(f.cpu().numpy())
    assert ok and chi == 2
    r = (v.double().cpu() - torch.tensor([-0.4, 0.0, 0.0], dtype=torch.float64)).norm(dim=1)
    assert (r - 0.45).abs().max().item() < 0.01                                # the first sphere, all of it, nothing else
    vol = M.volume(M.two_spheres_sdf, shape, org, spc)
    blocks, rounds = S.closure(vol, [(0, 2, 2)])
    assert (info["rounds"], info["cell_active_bricks"]) == (rounds, len(blocks))
    with pytest.raises(RuntimeError, match="1 rounds"):
        sparse_level_set(_two_spheres_torch, shape, org, spc, axes=axes, band=0, seeds=seed, max_rounds=1)
    # band seeding on an exact distance covers both spheres: the dense mesh of the same samples
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    dense = _two_spheres_torch(pts).reshape(shape)
    want_v, want_f = marching_tetrahedra(dense, org, spc)
    for band in (1.0, 1.5):
        v, f, vk, fc, info = sparse_level_set(_two_spheres_torch, shape, org, spc, axes=axes, band=band, return_info=True,
                                              return_keys=True)
        print("band %.1f: %r" % (band, info))
        got_v, got_f = _sorted_np(v, f, vk, fc)
        assert np.array_equal(got_f, want_f.cpu().numpy())
        assert np.array_equal(got_v.view(np.int32), want_v.cpu().numpy().view(np.int32))
        assert info["rounds"] == 1 and info["points_evaluated"] < 40 ** 3
    # origin and spacing without axes place the same points
    v2, f2 = sparse_level_set(_two_spheres_torch, shape, org, spc, band=1.0)
    assert torch.equal(f2, f) and (v2 - v).abs().max().item() < 1e-6
    nothing = sparse_level_set(_two_spheres_torch, shape, org, spc, band=0, return_info=True)
    assert nothing[0].shape == (0, 3) and nothing[1].shape == (0, 3) and nothing[2]["rounds"] == 0


def test_past_the_dense_limit(dev):
    """1537 points per side: a sphere of radius 0.1 in a box of side 2, h = 2 / 1536, r / h = 76.8.  The area bound is the
    float64 restatement's error at 193 per side (module docstring) scaled by h^2 and doubled."""
    from iso_points_amd.ops import marching_tetrahedra, sparse_level_set
    n, r = 1537, 0.1
    h = 2.0 / (n - 1)

    def sdf(x):
        return torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - r
    with pytest.raises(ValueError):
        marching_tetrahedra(torch.zeros((2, 2, n), device=dev))
    v, f, info = sparse_level_set(sdf, (n, n, n), (-1.0,) * 3, (h,) * 3, return_info=True)
    print("1537^3: %d vertices, %d faces, %r" % (v.shape[0], f.shape[0], info))
    assert info["points_evaluated"] < 0.01 * n ** 3 and info["sampled_bricks"] * 512 < info["points_evaluated"]
    faces, verts = f.cpu().numpy(), v.cpu().numpy().astype(np.float64)
    ok, chi = _closed_oriented_chi(faces)
    assert ok and chi == 2 and sorted(np.unique(faces)) == list(range(len(verts)))
    assert np.abs(np.linalg.norm(verts, axis=1) - r).max() < h
    normal, area = M.face_normals_areas(verts, faces)
    assert ((normal * verts[faces].mean(1)).sum(1) > 0).all()                  # outwards
    err = area.sum() / (4 * math.pi * r * r) - 1
    bound = 2 * SPHERE01_AREA_ERR_F64 * (h / SPHERE01_H0) ** 2
    print("area error %.3e, bound %.3e" % (err, bound))
    assert abs(err) <= bound


def test_the_largest_grid_from_one_seed(dev):
    """4096 points per side, the limit: the 512 MB brick table and point indices up to 2^36 in the keys.  A sphere of radius
    0.02 near the far corner of the box, found from one seed point by the closure alone (band seeding would evaluate
    512^3 test points)."""
    from iso_points_amd.ops import sparse_level_set
    n, r, c = 4096, 0.02, 0.9
    h = 2.0 / (n - 1)

    def sdf(x):
        dx, dy, dz = x[:, 0] - c, x[:, 1] - c, x[:, 2] - c
        return torch.sqrt(dx * dx + dy * dy + dz * dz) - r
    seed = torch.tensor([[c + r, c, c]], device=dev)
    v, f, vk, fc, info = sparse_level_set(sdf, (n, n, n), (-1.0,) * 3, (h,) * 3, band=0, seeds=seed, return_info=True,
                                          return_keys=True)
    print("4096^3: %d vertices, %d faces, %r" % (v.shape[0], f.shape[0], info))
    assert info["rounds"] > 2 and info["points_evaluated"] == 512 * info["sampled_bricks"] < 1e-4 * n ** 3
    assert info["workspace_bytes"] > 4 * 512 ** 3
    ok, chi = _closed_oriented_chi(f.cpu().numpy())
    assert f.shape[0] > 100000 and ok and chi == 2
    centre = torch.tensor([c, c, c], dtype=torch.float64)
    assert ((v.double().cpu() - centre).norm(dim=1) - r).abs().max().item() < h
    # the keys name the owning grid point: the vertex lies on a slot that starts there
    p = vk.cpu() // 7
    owner = torch.stack([p // (n * n), (p // n) % n, p % n], dim=1).double() * h - 1.0
    d = v.double().cpu() - owner
    assert d.min().item() > -1e-6 and d.max().item() < h + 1e-6 and int(p.max()) > 2 ** 35
    assert torch.equal(torch.sort(vk)[0], torch.unique(vk)) and int(fc.max()) > 2 ** 35


def test_fused_siren_samples_are_the_dense_volume(dev):
    """The 64 x 2 SIREN of test_sdf_grid_on_a_small_siren on 33^3: a brick's samples are the bits of sdf_grid's volume at
    the same points (each point is one row of the fused kernel), and then the meshes agree."""
    from iso_points_amd import ops
    from iso_points_amd.sdf_models import Siren
    torch.manual_seed(5)
    model = Siren(hidden_size=64, n_layers=2).to(dev)
    n = 33
    axis = torch.from_numpy((np.linspace(-0.5, 0.5, n) * 2.0).astype(np.float32)).to(dev)
    pts = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1)
    with torch.no_grad():
        model.net[-1].bias -= model(pts.reshape(-1, 3)).sdf.mean()
    values, origin, spacing = ops.sdf_grid(model, n, box_side_length=2.0)
    bricks = S.all_blocks((n, n, n))
    lin = torch.tensor([S.brick_lin(b, (n, n, n)) for b in bricks], dtype=torch.int64, device=dev)
    samples = ops._sdf_values(model, ops._brick_points(lin, [5, 5, 5], [n, n, n], [axis] * 3, None, None)).reshape(-1, 8, 8, 8)
    want = torch.from_numpy(S.to_bricks(values.cpu().numpy(), bricks)).to(dev)
    inside_grid = ~torch.isnan(want)
    assert inside_grid.sum().item() == n ** 3
    assert torch.equal(samples[inside_grid].view(torch.int32), want[inside_grid].view(torch.int32))
    want_v, want_f = ops.marching_tetrahedra(values, origin, spacing)
    v, f, vk, fc, info = ops.sparse_level_set(model, (n, n, n), origin, spacing, axes=[axis] * 3, band=1e9, return_keys=True,
                                              return_info=True)
    assert info["cell_active_bricks"] == 64 and info["sampled_bricks"] == 125 and info["rounds"] == 1
    got_v, got_f = _sorted_np(v, f, vk, fc)
    print("siren 64 x 2 on 33^3: %d vertices, %d faces" % (len(got_v), len(got_f)))
    assert len(got_f) > 100 and np.array_equal(got_f, want_f.cpu().numpy())
    assert np.array_equal(got_v.view(np.int32), want_v.cpu().numpy().view(np.int32))
    # the closure alone, from the centroid of one dense face: the component it lies on, a subset of the dense vertices
    seed = want_v[want_f[0]].mean(dim=0, keepdim=True)
    v1, f1, vk1, fc1, info1 = ops.sparse_level_set(model, (n, n, n), origin, spacing, axes=[axis] * 3, band=0, seeds=seed,
                                                   return_keys=True, return_info=True)
    assert info1["rounds"] > 1 and 0 < f1.shape[0] <= want_f.shape[0]
    assert np.isin(vk1.cpu().numpy(), vk.cpu().numpy()).all()


def test_high_res_mesh_sparse(dev):
    """get_surface_high_res_mesh(SphereSDF, 48, sparse=True): closed, and as close to the exact sphere as the dense chain is
    asked to be (twice the float64 restatement's documented Chamfer distance); sparse=False is the default path."""
    from iso_points_amd.loss import chamfer_distance
    from iso_points_amd.ops import get_surface_high_res_mesh, sample_points_from_meshes
    from iso_points_amd.sdf_models import SphereSDF
    radius = 0.6
    sdf = SphereSDF(radius=radius).to(dev)
    gen = torch.Generator().manual_seed(11)
    verts, faces, normals = get_surface_high_res_mesh(sdf, resolution=48, return_normals=True, generator=gen, sparse=True)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64 and verts.is_cuda and faces.is_cuda
    ok, chi = _closed_oriented_chi(faces.cpu().numpy())
    assert faces.shape[0] > 5000 and ok and chi == 2
    assert ((normals * verts / verts.norm(dim=1, keepdim=True)).sum(1) > 0.999).all()
    cloud = sample_points_from_meshes((verts[None], faces[None]), 10000, generator=gen)
    g = torch.Generator().manual_seed(12)
    exact = torch.nn.functional.normalize(torch.randn(1, 10000, 3, generator=g), dim=-1).to(dev) * radius
    cham = chamfer_distance(cloud, exact)[0].item()
    print("chamfer distance of the sparse chain's sphere: %.4e (float64 restatement's dense chain: %.4e)" % (cham, CHAIN_CHAMFER_F64))
    assert cham <= 2 * CHAIN_CHAMFER_F64
    dense = get_surface_high_res_mesh(sdf, resolution=48, generator=torch.Generator().manual_seed(11))
    again = get_surface_high_res_mesh(sdf, resolution=48, generator=torch.Generator().manual_seed(11), sparse=False)
    assert torch.equal(dense[0], again[0]) and torch.equal(dense[1], again[1])
    # the same surface on the same aligned grid: the two paths evaluate the rotated points in different batches, so their
    # meshes are compared by size (a flag may differ where a sample is within rounding of the level), not by bits
    assert abs(dense[1].shape[0] - faces.shape[0]) <= 0.001 * faces.shape[0]


def test_two_runs_and_a_side_stream_give_the_same_bits(dev):
    from iso_points_amd.ops import marching_tetrahedra_bricks, sparse_level_set
    vol, org, spc, level = case("sphere33")[:4]
    active = _subsets("sphere33")["half"]
    bricks = S.sampled(active, vol.shape)
    values, coords, flags = _bricked(vol, bricks, active, dev)
    shape, sorg, sspc = SPLIT_GRID

    def both():
        a = marching_tetrahedra_bricks(values, coords, flags, vol.shape, org, spc, level, return_keys=True, return_need=True)
        b = sparse_level_set(_two_spheres_torch, shape, sorg, sspc, band=0, seeds=torch.tensor([[-0.85, 0.0, 0.0]], device=dev))
        return a + b
    first, second = both(), both()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both()
    side.synchronize()
    for other in (second, third):
        for x, y in zip(first, other):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert first[1].shape[0] > 0 and first[6].shape[0] > 0


def test_refusals_through_the_abi(dev):
    from iso_points_amd import _lib
    from iso_points_amd.ops import marching_tetrahedra_bricks
    lib = _lib.load()
    n = 12
    vol, org, spc, level = _boxed(lambda p: M.sphere_sdf(p, 0.6), n)
    bricks = S.all_blocks(vol.shape)
    values, coords, flags = _bricked(vol, bricks, bricks, dev)
    Sn = len(bricks)
    ws_bytes = lib.iso_meshextract_sparse_workspace_bytes(n, n, n, Sn)
    assert ws_bytes > 17 * 512 * Sn and ws_bytes % 16 == 0
    for bad in ((1, n, n, Sn), (n, 4097, n, Sn), (n, n, n, 0), (n, n, n, 1 << 22)):
        assert lib.iso_meshextract_sparse_workspace_bytes(*bad) == 0, bad
    assert lib.iso_meshextract_sparse_workspace_bytes(4096, 4096, 4096, 1) > 4 * 512 ** 3
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    need = torch.full((Sn,), 77, dtype=torch.uint8, device=dev)
    totals = torch.full((4,), -1, dtype=torch.int64, device=dev)
    p, s = _lib.ptr, _lib.stream()

    def count(vals=values, co=coords, act=flags, S_=Sn, dims=(n, n, n), iso=0.0, nd=need, tot=totals, work=ws, nbytes=ws_bytes):
        return lib.iso_meshextract_sparse_count(p(vals), p(co), p(act), S_, dims[0], dims[1], dims[2], iso, p(nd), p(tot), p(work),
                                                nbytes, s)
    for dims in ((1, n, n), (n, 1, n), (n, n, 1), (0, n, n), (-3, n, n)):
        assert count(dims=dims) == INVALID, dims
    for dims in ((4097, n, n), (n, 4097, n), (n, n, 4097)):
        assert count(dims=dims) == UNSUPPORTED, dims
    assert count(S_=0) == INVALID and count(S_=-1) == INVALID
    assert count(S_=1 << 22) == UNSUPPORTED                                          # S * 512 = 2^31
    assert count(vals=None) == INVALID and count(co=None) == INVALID and count(act=None) == INVALID
    assert count(nd=None) == INVALID and count(tot=None) == INVALID and count(work=None) == INVALID
    assert count(iso=float("nan")) == INVALID
    assert count(nbytes=ws_bytes - 16) == WORKSPACE
    assert b"iso_meshextract_sparse_count" in lib.iso_last_error()
    torch.cuda.synchronize()
    assert (need == 77).all() and (totals == -1).all()                               # a refused call writes nothing
    assert count() == 0
    V, F, n_need, n_out = totals.tolist()
    want_v, want_f = M.extract(vol, org, spc)
    assert (V, F, n_need, n_out) == (len(want_v), len(want_f), 0, 0) and V > 0 and F > 0
    verts = torch.full((V + 1, 3), -7.0, device=dev)
    faces = torch.full((F + 1, 3), -7, dtype=torch.int32, device=dev)

    def emit(vals=values, co=coords, S_=Sn, dims=(n, n, n), spacing=spc, tot=totals, v=verts, vcap=V, f=faces, fcap=F, work=ws,
             nbytes=ws_bytes):
        return lib.iso_meshextract_sparse_emit(p(vals), p(co), p(flags), S_, dims[0], dims[1], dims[2], org[0], org[1], org[2],
                                               spacing[0], spacing[1], spacing[2], 0.0, p(tot), p(v), vcap, p(f), fcap, None, None,
                                               p(work), nbytes, s)
    assert emit(vcap=V - 1) == INVALID and emit(fcap=F - 1) == INVALID and emit(vcap=0, fcap=0) == INVALID      # outputs too small
    assert emit(vcap=-1) == INVALID
    assert emit(dims=(1, n, n)) == INVALID and emit(dims=(n, n, 4097)) == UNSUPPORTED and emit(S_=1 << 22) == UNSUPPORTED
    assert emit(vals=None) == INVALID and emit(co=None) == INVALID and emit(tot=None) == INVALID and emit(work=None) == INVALID
    assert emit(v=None) == INVALID and emit(f=None) == INVALID
    assert emit(spacing=(0.0, 0.4, 0.4)) == INVALID
    assert emit(nbytes=ws_bytes - 16) == WORKSPACE
    for many in ([1 << 31, 0, 0, 0], [0, 1 << 31, 0, 0]):                                                         # 2^31 of either
        assert emit(tot=torch.tensor(many, dtype=torch.int64, device=dev), vcap=1 << 32, fcap=1 << 32) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (verts == -7.0).all() and (faces == -7).all()
    assert emit() == 0
    torch.cuda.synchronize()
    assert (verts[V:] == -7.0).all() and (faces[F:] == -7).all()                     # nothing beyond the totals
    assert int(faces[:F].min()) == 0 and int(faces[:F].max()) == V - 1
    # coords outside the grid: the count reports them and counts nothing for them, the emit refuses
    outside = coords.clone()
    outside[3] = torch.tensor([0, 2, 0], dtype=torch.int32)                          # 12 points: bricks 0 and 1 per axis
    tot2 = torch.zeros((4,), dtype=torch.int64, device=dev)
    assert count(co=outside, tot=tot2) == 0
    assert tot2[3].item() == 1
    verts.fill_(-7.0)
    assert emit(co=outside, tot=tot2, vcap=V + 1, fcap=F + 1) == INVALID
    assert b"outside the grid" in lib.iso_last_error()
    negative = coords.clone()
    negative[0, 2] = -1
    assert count(co=negative, tot=tot2) == 0 and tot2[3].item() == 1
    torch.cuda.synchronize()
    assert (verts == -7.0).all()
    # the package checks the list before anything is launched
    with pytest.raises(RuntimeError, match="no CPU path"):
        marching_tetrahedra_bricks(values.cpu(), coords.cpu(), flags.cpu(), vol.shape)
    with pytest.raises(ValueError, match="outside the grid"):
        marching_tetrahedra_bricks(values, outside, flags, vol.shape)
    with pytest.raises(ValueError, match="twice"):
        marching_tetrahedra_bricks(values, torch.cat([coords[:-1], coords[:1]]), flags, vol.shape)
    with pytest.raises(ValueError, match="lacks"):
        marching_tetrahedra_bricks(values[:-1], coords[:-1], flags[:-1], vol.shape)
    with pytest.raises(ValueError):
        marching_tetrahedra_bricks(values, coords, flags, (n, n, 4097))
    with pytest.raises(ValueError):
        marching_tetrahedra_bricks(values[:, :4], coords, flags, vol.shape)
