"""iso_points_amd.mesh_raster on the GPU against the numpy oracle of tests/mesh_raster_oracle.py (brute force over all
(pixel, face) pairs in float64; the rule is include/isopoints.h section M).

pix_to_face is compared EXACTLY on every safe pixel (the oracle's module docstring defines them; unsafe pixels are capped at
1 % of a scene's covered pixels, checked without a GPU in tests/test_mesh_raster_cpu.py) and on every pixel of the scenes
with dyadic coordinates, where float32 is exact.  Empty slots hold exactly -1 in all four outputs.

Bound for zbuf, bary_coords and dists on the slots whose face matches: |got - ref| <= A, nothing relative.  A never comes
from the kernel: the oracle's float32 restatement runs on the inputs of the test at hand, and A is 4 x its largest error
against float64, the error taken as at least half a float32 step at the largest reference entry.  Measured on the CPU
(largest float32 error -> A), camera look_at_view(2.7, 20, 30) / perspective(60):
    icosphere(2) S = 48   zbuf 2.3e-06 -> 9.3e-06   bary 8.3e-07 -> 3.3e-06   dists 2.5e-09 -> 9.8e-09
      perspective-correct zbuf 4.9e-07 -> 1.9e-06   bary 2.9e-07 -> 1.1e-06
    icosphere(2) S = 33   zbuf 1.2e-06 -> 4.7e-06   bary 5.1e-07 -> 2.0e-06   dists 2.5e-09 -> 9.9e-09
    icosphere(3) S = 48   zbuf 1.1e-06 -> 4.5e-06   bary 7.9e-07 -> 3.1e-06   dists 1.1e-09 -> 4.5e-09
    icosphere(3) S = 33   zbuf 1.4e-06 -> 5.6e-06   bary 3.0e-07 -> 1.2e-06   dists 1.2e-09 -> 5.0e-09
(depths are 1.7 .. 3.6: a relative depth error of the restatement of 1.6e-07 .. 9.4e-07).  Unsafe pixels there: 0 or 1 of
402 .. 864 covered."""
import numpy as np
import pytest
import torch

import mesh_raster_oracle as O

pytestmark = pytest.mark.gpu


def run(dev, face_verts, first, num, S, K, persp=False, cull=False):
    from iso_points_amd.ops import rasterize_meshes
    fr = rasterize_meshes(O.PackedMeshes(face_verts, first, num, dev), image_size=S, faces_per_pixel=K,
                          perspective_correct=persp, cull_backfaces=cull)
    N = len(first)
    assert fr.pix_to_face.dtype == torch.int64 and fr.pix_to_face.shape == (N, S, S, K)
    assert fr.zbuf.dtype == fr.bary_coords.dtype == fr.dists.dtype == torch.float32
    assert fr.zbuf.shape == fr.dists.shape == (N, S, S, K) and fr.bary_coords.shape == (N, S, S, K, 3)
    assert not any(t.requires_grad for t in fr)
    return fr


def as_numpy(fr):
    return dict(pix_to_face=fr.pix_to_face.cpu().numpy(), zbuf=fr.zbuf.cpu().numpy(), bary=fr.bary_coords.cpu().numpy(),
                dists=fr.dists.cpu().numpy())


def compare(fr, r64, r32, every_pixel=False, what=""):
    """The checks of the module docstring; returns the numpy outputs."""
    got = as_numpy(fr)
    unsafe = np.zeros_like(r64["unsafe"]) if every_pixel else r64["unsafe"]
    covered = int(r64["covered"].sum())
    n_unsafe = int((unsafe & r64["covered"]).sum())
    print("%s: %d covered pixels, %d unsafe" % (what, covered, n_unsafe))
    assert n_unsafe <= O.UNSAFE_CAP * covered, (what, n_unsafe, covered)
    safe = ~unsafe
    bad = (got["pix_to_face"] != r64["pix_to_face"]).any(-1) & safe
    assert not bad.any(), "%s: pix_to_face differs on %d safe pixels, first at %s: got %s, oracle %s" % (
        what, int(bad.sum()), np.argwhere(bad)[0], got["pix_to_face"][bad][0], r64["pix_to_face"][bad][0])
    A, errs = O.bounds(r64, r32)
    hit = (r64["pix_to_face"] >= 0) & safe[..., None]
    empty = (r64["pix_to_face"] < 0) & safe[..., None]
    for name in ("zbuf", "bary", "dists"):
        g, ref = got[name].astype(np.float64), r64[name]
        m = np.broadcast_to(hit[..., None] if name == "bary" else hit, g.shape)
        e = np.broadcast_to(empty[..., None] if name == "bary" else empty, g.shape)
        worst = float(np.abs(g - ref)[m].max()) if m.any() else 0.0
        print("  %s: restatement error %.3g -> A = %.3g; kernel's largest |d| = %.3g" % (name, errs[name], A[name], worst))
        assert worst <= A[name], (what, name, worst, A[name])
        assert (g[e] == -1.0).all(), (what, name)
    # ascending (pz, face) order, empty slots last
    z, f = got["zbuf"], got["pix_to_face"]
    for j in range(z.shape[-1] - 1):
        both = (f[..., j] >= 0) & (f[..., j + 1] >= 0)
        assert (f[..., j + 1] < 0)[f[..., j] < 0].all()
        assert ((z[..., j] < z[..., j + 1]) | ((z[..., j] == z[..., j + 1]) & (f[..., j] < f[..., j + 1])))[both].all(), what
    return got


@pytest.mark.parametrize("level,S,persp", O.SPHERE_CASES)
def test_spheres(dev, level, S, persp):
    fv, r64, r32 = O.sphere_reference(level, S, persp)
    fr = run(dev, fv, [0], [len(fv)], S, O.SPHERE_K, persp)
    got = compare(fr, r64, r32, what="icosphere(%d) S = %d persp %s" % (level, S, persp))
    assert r64["covered"].sum() > 300 and (r64["pix_to_face"][..., 1] >= 0).sum() > 300      # two layers ...
    assert (got["pix_to_face"][..., 2:] == -1).all() and (got["zbuf"][..., 2:] == -1).all()    # ... and no third
    assert (got["bary"][..., 2:, :] == -1).all() and (got["dists"][..., 2:] == -1).all()


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8])
def test_stack_of_parallel_triangles_every_pixel(dev, K):
    """Dyadic coordinates: float32 is exact, every pixel is compared.  Truncation to the K nearest, the tie rule and the
    centres that lie exactly on a shared edge or vertex."""
    from iso_points_amd import _lib
    assert _lib.load().iso_meshraster_form(K) == {1: 1, 2: 4, 3: 4, 4: 4, 5: 8, 8: 8}[K]
    fv = O.stack_scene()
    r64 = O.rasterize(fv, [0], [len(fv)], 32, K)
    r32 = O.rasterize(fv, [0], [len(fv)], 32, K, dtype=np.float32)
    got = compare(run(dev, fv, [0], [len(fv)], 32, K), r64, r32, every_pixel=True, what="stack K = %d" % K)
    f = got["pix_to_face"][0]
    want = [10, 11, 9, 8, 7, 6, 5, 12]                        # centre pixel: the equal pair first (lower index first), then
    assert f[16, 16].tolist() == want[:K]                     # the stack from its last face (nearest) backwards
    full = O.rasterize(fv, [0], [len(fv)], 32, 8)["pix_to_face"][0]
    assert (f == full[..., :K]).all()                         # K nearest = the first K of a longer list
    # the split quad (faces 14, 15): its corner pixels (31, 31), (23, 23), its outline and its diagonal belong to neither
    quad = np.isin(f, (14, 15)).any(-1)
    assert quad.sum() > 20 and not quad[np.arange(32), np.arange(32)].any()
    assert not quad[31].any() and not quad[:, 31].any() and not quad[23].any() and not quad[:, 23].any()
    assert f[29, 30, 0] == 15 and f[30, 29, 0] == 14          # either side of the diagonal, below the stack


@pytest.mark.parametrize("S", [1, 15, 16, 17, 31, 50])
def test_tile_edges(dev, S):
    fv = O.edge_scene()
    r64 = O.rasterize(fv, [0], [len(fv)], S, 3)
    r32 = O.rasterize(fv, [0], [len(fv)], S, 3, dtype=np.float32)
    got = compare(run(dev, fv, [0], [len(fv)], S, 3), r64, r32, what="edges S = %d" % S)
    assert (got["pix_to_face"][..., 1] >= 0).all()            # two faces cover every pixel of every tile
    assert not (got["pix_to_face"] == 3).any()                # the off-screen face is nowhere
    if S >= 15:
        assert (got["pix_to_face"] == 2).any() and (got["pix_to_face"][..., 0] == 4).any()


def test_skipped_faces_and_pairs(dev):
    fv = O.skip_scene()
    r64 = O.rasterize(fv, [0], [len(fv)], 40, 4)
    r32 = O.rasterize(fv, [0], [len(fv)], 40, 4, dtype=np.float32)
    got = compare(run(dev, fv, [0], [len(fv)], 40, 4), r64, r32, what="skips")
    f = got["pix_to_face"]
    assert (f == 0).any() and not np.isin(f, (1, 2, 3)).any()
    assert (f == 4).any() and (got["zbuf"][f == 4] >= 0).all()
    lifted = fv[4:].copy()                                    # the last face alone with |z|: the same outline, every pz > 0
    lifted[..., 2] = np.abs(lifted[..., 2])
    outline = O.rasterize(lifted, [0], [1], 40, 1)["covered"][0]
    kept = (f[0] == 4).any(-1)
    assert outline.sum() > kept.sum() > 0 and not (kept & ~outline).any()       # part of its pixels has pz < 0: dropped


@pytest.mark.parametrize("persp", [False, True])
def test_cull_backfaces_on_the_sphere(dev, persp):
    fv, r64, _ = O.sphere_reference(2, 48, persp)
    _, c64, c32 = O.sphere_reference(2, 48, persp, True)
    got = compare(run(dev, fv, [0], [len(fv)], 48, O.SPHERE_K, persp, cull=True), c64, c32, what="culled sphere")
    assert (got["pix_to_face"][..., 1:] == -1).all()
    safe = ~r64["unsafe"][0]
    assert (got["pix_to_face"][0, ..., 0][safe] == r64["pix_to_face"][0, ..., 0][safe]).all()


def test_heavy_tile_and_face_order(dev):
    """3001 faces in one tile: twelve LDS chunks.  The nearest face is stored last; the reversed list gives the same image."""
    fv = O.heavy_tile_scene()
    F = len(fv)
    r64 = O.rasterize(fv, [0], [F], 32, 4)
    r32 = O.rasterize(fv, [0], [F], 32, 4, dtype=np.float32)
    fr = run(dev, fv, [0], [F], 32, 4)
    got = compare(fr, r64, r32, what="heavy tile")
    assert (got["pix_to_face"][0, :16, :16, 0] == F - 1).all() and (got["pix_to_face"][0, :16, :16, 3] >= 0).mean() > 0.5
    rev = as_numpy(run(dev, fv[::-1].copy(), [0], [F], 32, 4))
    mapped = np.where(rev["pix_to_face"] >= 0, F - 1 - rev["pix_to_face"], -1)
    assert (mapped == got["pix_to_face"]).all()
    for name in ("zbuf", "bary", "dists"):
        assert (rev[name].view(np.uint32) == got[name].view(np.uint32)).all(), name


def test_batch_of_three_meshes_packed_indices(dev):
    """320, 0 and 20 faces: pix_to_face holds packed indices, the empty mesh's image is empty."""
    big, _ = O.sphere_faces(2)
    small, _ = O.sphere_faces(0)
    fv = np.concatenate([big, small])
    first, num = [0, 320, 320], [320, 0, 20]
    r64 = O.rasterize(fv, first, num, 33, 3)
    r32 = O.rasterize(fv, first, num, 33, 3, dtype=np.float32)
    got = compare(run(dev, fv, first, num, 33, 3), r64, r32, what="batch")
    f = got["pix_to_face"]
    assert (f[0] < 320).all() and (f[0] >= 0).any() and (f[1] == -1).all()
    assert ((f[2] == -1) | (f[2] >= 320)).all() and (f[2] >= 320).any()
    # the padded tuple form with face counts gives the same fragments
    from iso_points_amd.ops import rasterize_meshes
    verts = torch.zeros(3, 960, 3)
    faces = torch.zeros(3, 320, 3, dtype=torch.int64)
    verts[0] = torch.from_numpy(big.reshape(-1, 3))
    verts[2, :60] = torch.from_numpy(small.reshape(-1, 3))
    faces[0] = torch.arange(960).reshape(320, 3)
    faces[2, :20] = torch.arange(60).reshape(20, 3)
    fr = rasterize_meshes((verts.to(dev), faces.to(dev), torch.tensor([320, 0, 20])), image_size=33, faces_per_pixel=3)
    for a, b in zip(as_numpy(fr).values(), got.values()):
        assert (a == b).all()


def test_one_mesh_three_cameras_through_the_rasterizer(dev):
    from iso_points_amd import cameras
    from iso_points_amd.ops import MeshRasterizer, RasterizationSettings
    v, f = O.icosphere(2)
    views = torch.stack([cameras.look_at_view(2.7, 20.0, 30.0), cameras.look_at_view(3.0, -10.0, 100.0),
                         cameras.look_at_view(2.5, 60.0, 250.0)])
    projs = views @ cameras.perspective(60.0)
    rast = MeshRasterizer((views.to(dev), projs.to(dev)), RasterizationSettings(image_size=33, faces_per_pixel=2))
    mesh = (torch.from_numpy(v)[None].to(dev), torch.from_numpy(f)[None].to(dev))
    ndc, first, num, _ = rast.transform(mesh)
    assert ndc.shape == (960, 3, 3) and first.tolist() == [0, 320, 640] and num.tolist() == [320, 320, 320]
    fr = rast(mesh)
    r64 = O.rasterize(ndc.cpu().numpy(), first.tolist(), num.tolist(), 33, 2)
    r32 = O.rasterize(ndc.cpu().numpy(), first.tolist(), num.tolist(), 33, 2, dtype=np.float32)
    got = compare(fr, r64, r32, what="three cameras")
    for n in range(3):
        fn = got["pix_to_face"][n]
        assert (fn >= 0).sum() > 300 and ((fn < 0) | ((fn >= 320 * n) & (fn < 320 * (n + 1)))).all()
    # the torch transform against the float32 numpy one on the first camera
    ref = O.to_ndc(v, views[0].numpy(), projs[0].numpy())[f]
    assert np.abs(ndc[:320].cpu().numpy() - ref).max() < 1e-5


def test_two_runs_are_bit_identical(dev):
    for level, S, persp in O.SPHERE_CASES:
        fv, _, _ = O.sphere_reference(level, S, persp)
        a = as_numpy(run(dev, fv, [0], [len(fv)], S, O.SPHERE_K, persp))
        b = as_numpy(run(dev, fv, [0], [len(fv)], S, O.SPHERE_K, persp))
        assert (a["pix_to_face"] == b["pix_to_face"]).all()
        for name in ("zbuf", "bary", "dists"):
            assert (a[name].view(np.uint32) == b[name].view(np.uint32)).all(), name


def test_render_views_mask_and_depth(dev):
    from iso_points_amd import cameras
    from iso_points_amd.ops import MeshRasterizer, render_views
    v, f = O.icosphere(2)
    view = cameras.look_at_view(2.7, 20.0, 30.0)[None]
    cams = (view.to(dev), (view @ cameras.perspective(60.0)).to(dev))
    mesh = (torch.from_numpy(v)[None].to(dev), torch.from_numpy(f)[None].to(dev))
    out = render_views(mesh, cams, image_size=48, faces_per_pixel=5, zfar=100.0, light_location=(2.0, 2.0, 2.0))
    assert out.images.shape == (1, 48, 48, 4) and out.mask.shape == out.depth.shape == (1, 48, 48, 1)
    assert out.mask.dtype == torch.uint8 and not out.images.requires_grad
    ndc, first, num, world = MeshRasterizer(cams).transform(mesh)
    r64 = O.rasterize(ndc.cpu().numpy(), [0], [320], 48, 5)
    r32 = O.rasterize(ndc.cpu().numpy(), [0], [320], 48, 5, dtype=np.float32)
    compare(out.fragments, r64, r32, what="render_views")
    safe = ~r64["unsafe"]
    mask = out.mask.cpu().numpy()[..., 0]
    assert set(np.unique(mask)) == {0, 255} and ((mask == 255) == r64["covered"])[safe].all()
    depth = out.depth.cpu().numpy()[..., 0].astype(np.float64)
    ref = np.where(r64["covered"], r64["zbuf"][..., 0], 100.0)
    A, _ = O.bounds(r64, r32)
    assert (np.abs(depth - ref)[safe] <= A["zbuf"]).all() and (depth[safe & ~r64["covered"]] == 100.0).all()
    img = out.images.cpu().numpy()
    assert (img[..., 3] == (mask == 255)).all() and (img[..., :3][mask == 0] == 1.0).all()
    shade = O.flat_shading(r64["pix_to_face"][..., 0], r64["bary"][..., 0, :], world.cpu().numpy(),
                           np.linalg.inv(view[0].numpy().astype(np.float64))[3, :3], light_location=(2.0, 2.0, 2.0))
    # float32 torch against float64 numpy of the same formula: the barycentrics differ by at most A["bary"] (3e-6), unit
    # vectors and cosines by a few float32 steps of 1 (6e-8 each, ~1e-6 after normalising twice), and the specular term
    # cos^64 amplifies its argument's error 64-fold at most: 0.2 * 64 * 4e-6 = 5e-5.  1e-4 leaves a factor of two.
    assert np.abs(img.astype(np.float64) - shade)[safe].max() < 1e-4
