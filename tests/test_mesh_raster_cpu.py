"""Mesh rasterisation without a GPU: the module imports, every argument error is raised before any GPU call, the header,
the ctypes table and the built library agree on the iso_meshraster_* entries, every refusal of the C entries returns
non-zero without a launch, and the numpy oracle of tests/mesh_raster_oracle.py is checked on its own: the float32
restatement equals float64 on safe pixels, the 1 % cap on unsafe pixels holds on every scene tests/test_mesh_raster_gpu.py
uses, culling leaves the sphere's front layer, and an axis-aligned triangle has the coverage and barycentrics of the
analytic answer.  hard_flat_shading and render_views are plain torch and run here against a float64 numpy restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_raster_oracle as O

ENTRIES = ("iso_meshraster_form", "iso_meshraster_count", "iso_meshraster_fill", "iso_meshraster_pixels")
CITES = ("scripts/create_mvr_data_from_mesh.py:143-216", "DSS/training/losses.py:550-578", "tests/test_data.py",
         "tests/test_dvr_camera.py")


def test_the_module_imports_without_a_gpu():
    from iso_points_amd import mesh_raster, ops
    for name in ("Fragments", "rasterize_meshes", "RasterizationSettings", "MeshRasterizer", "hard_flat_shading", "render_views"):
        assert getattr(ops, name) is getattr(mesh_raster, name), name
    assert mesh_raster.Fragments._fields == ("pix_to_face", "zbuf", "bary_coords", "dists")
    rs = mesh_raster.RasterizationSettings()
    assert rs.blur_radius == 0.0 and rs.bin_size is None and rs.max_faces_per_bin is None


def test_header_table_and_library_agree_on_the_mesh_raster_entries():
    import test_abi
    from iso_points_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(s for s in declared if s.startswith("iso_meshraster_")) == sorted(ENTRIES)
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("iso_meshraster_")) == sorted(ENTRIES)
    txt = re.sub(r"/\*.*?\*/", "", open(test_abi.HEADER).read(), flags=re.S)
    for name in ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_section_m_follows_l_and_cites_the_call_sites():
    import test_abi
    head = open(test_abi.HEADER).read()
    title = "M. Mesh rasterisation: faces, depth and barycentrics per pixel (csrc/mesh_raster.hip)"
    assert head.index("L. Even sampling: Poisson-disk elimination (csrc/disk.hip)") < head.index(title)
    section = head.split(title)[1]
    for cite in CITES:
        assert cite in section, cite


def test_the_new_file_is_built_once_without_the_slp_vectoriser():
    import subprocess
    import test_abi
    root = os.path.dirname(os.path.dirname(test_abi.HEADER))
    out = subprocess.run(["make", "-n", "-B", "-C", root, "iso_points_amd/libisopoints_hip.so"], stdout=subprocess.PIPE,
                         text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and "mesh_raster.hip" in l]
    assert len(lines) == 1 and "-fno-slp-vectorize" in lines[0].split(), lines


def test_every_refusal_returns_an_error_without_a_gpu():
    from iso_points_amd import _lib
    lib = _lib.load()
    assert [lib.iso_meshraster_form(k) for k in range(0, 10)] == [0, 1, 4, 4, 4, 8, 8, 8, 8, 0]
    x = ctypes.c_void_p(16)          # a non-null pointer that is never followed: every call below returns before a launch

    def count(n=1, f=10, s=32, ptr=x):
        return lib.iso_meshraster_count(ptr, ptr, ptr, n, f, s, 0, ptr, None)

    def fill(n=1, f=10, s=32, cap=5, ptr=x):
        return lib.iso_meshraster_fill(ptr, ptr, ptr, n, f, s, 0, ptr, ptr, ptr, cap, None)

    def pixels(n=1, f=10, s=32, k=4, cap=5, ptr=x):
        return lib.iso_meshraster_pixels(ptr, n, f, s, k, 0, ptr, ptr, cap, ptr, ptr, ptr, ptr, None)

    # nothing to do is not an error
    assert count(n=0) == 0 and count(f=0) == 0 and count(n=0, ptr=None) == 0 and count(f=0, ptr=None) == 0
    assert fill(n=0) == 0 and fill(f=0) == 0 and fill(cap=0, ptr=None) == 0
    assert pixels(n=0) == 0 and pixels(n=0, ptr=None) == 0
    for k in (0, 9, -1, 150):                                                     # K outside 1..8
        assert pixels(k=k) != 0, k
    for s in (0, -5):                                                             # S < 1
        assert count(s=s) != 0 and fill(s=s) != 0 and pixels(s=s) != 0, s
    assert pixels(n=2, s=2 ** 14, k=4) != 0                                       # N * S * S * K = 2^31
    assert pixels(n=1, s=2 ** 15, k=2) != 0
    assert count(n=2 ** 15, s=2 ** 8) != 0                                        # (K = 1: the tile table's own limit)
    assert pixels(n=2 ** 30, s=2 ** 20, k=8) != 0                                 # a product beyond 64 bits
    for f in (2 ** 31, 2 ** 40):                                                  # F >= 2^31
        assert count(f=f) != 0 and fill(f=f) != 0 and pixels(f=f) != 0, f
    assert count(n=-1) != 0 and count(f=-1) != 0 and fill(n=-1) != 0 and fill(f=-1) != 0 and fill(cap=-1) != 0
    assert pixels(n=-1) != 0 and pixels(f=-1) != 0 and pixels(cap=-1) != 0
    assert count(ptr=None) != 0 and fill(ptr=None) != 0 and pixels(ptr=None) != 0   # null pointers where work exists
    assert pixels(cap=0, ptr=None) != 0                                           # (the outputs exist even without pairs)
    assert b"iso_meshraster_" in lib.iso_last_error()


def test_bad_arguments_raise_value_error():
    from iso_points_amd.ops import MeshRasterizer, RasterizationSettings, rasterize_meshes, render_views
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))
    mesh = (verts, faces)
    views = torch.eye(4)[None].repeat(3, 1, 1)
    for bad in (lambda: rasterize_meshes(mesh, blur_radius=1e-4),
                lambda: rasterize_meshes(mesh, blur_radius=None),
                lambda: rasterize_meshes(mesh, faces_per_pixel=0),
                lambda: rasterize_meshes(mesh, faces_per_pixel=9),
                lambda: rasterize_meshes(mesh, faces_per_pixel=2.0),
                lambda: rasterize_meshes(mesh, image_size=0),
                lambda: rasterize_meshes(mesh, image_size=-4),
                lambda: rasterize_meshes(mesh, image_size=32.0),
                lambda: rasterize_meshes(mesh, image_size=(32, 48)),
                lambda: rasterize_meshes(mesh, image_size=2 ** 14, faces_per_pixel=4),        # 2 * 2^28 * 4 = 2^31
                lambda: rasterize_meshes((verts,)),
                lambda: rasterize_meshes((verts, faces.float())),
                lambda: rasterize_meshes((verts[0], faces[0])),
                lambda: rasterize_meshes(object()),
                lambda: MeshRasterizer()(mesh),                                               # no cameras
                lambda: MeshRasterizer((views, views))(mesh),                                 # 2 meshes, 3 cameras
                lambda: MeshRasterizer((views, views[:2]))(mesh),
                lambda: MeshRasterizer((views[:2], views[:2]), RasterizationSettings(blur_radius=0.1))(mesh),
                lambda: MeshRasterizer((views[:2], views[:2]), RasterizationSettings(faces_per_pixel=16))(mesh),
                lambda: render_views(mesh, (views[:2], views[:2]), faces_per_pixel=0),
                lambda: render_views(mesh, (views[:2], views[:2]), fragments=object())):
        with pytest.raises(ValueError):
            bad()


def test_cpu_tensors_are_refused():
    from iso_points_amd.ops import MeshRasterizer, rasterize_meshes, render_views
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))
    views = torch.eye(4)[None].repeat(2, 1, 1)
    for fn in (lambda: rasterize_meshes((verts, faces)),
               lambda: rasterize_meshes((verts, faces), 16, 0.0, 1, None, None, True, True),
               lambda: rasterize_meshes(O.PackedMeshes(O.stack_scene(), [0], [16]), 32, faces_per_pixel=3),
               lambda: MeshRasterizer((views, views))((verts, faces)),
               lambda: render_views((verts, faces), (views, views), image_size=16)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


# ---------------------------------------------------------------------------------------------------------- the oracle
def cap_holds(r64, what):
    covered, unsafe = int(r64["covered"].sum()), int((r64["unsafe"] & r64["covered"]).sum())
    print("%s: %d unsafe of %d covered pixels" % (what, unsafe, covered))
    assert unsafe <= O.UNSAFE_CAP * covered, (what, unsafe, covered)


@pytest.mark.parametrize("level,S,persp", O.SPHERE_CASES)
def test_restatement_equals_float64_on_safe_pixels_of_the_spheres(level, S, persp):
    fv, r64, r32 = O.sphere_reference(level, S, persp)
    cap_holds(r64, "icosphere(%d) S = %d" % (level, S))
    safe = ~r64["unsafe"]
    assert (r64["pix_to_face"] == r32["pix_to_face"])[safe].all()
    A, errs = O.bounds(r64, r32)
    print("errors of the restatement %s -> A %s" % (errs, A))
    assert 0 < errs["zbuf"] < 1e-5 and 0 < errs["bary"] < 1e-5 and errs["dists"] < 1e-7
    assert 400 <= r64["covered"].sum() <= 870 and (r64["pix_to_face"][..., 2:] == -1).all()
    # front faces of the outward-wound sphere have area > 0, the back layer < 0
    area = (fv[:, 2, 0] - fv[:, 0, 0]) * (fv[:, 1, 1] - fv[:, 0, 1]) - (fv[:, 2, 1] - fv[:, 0, 1]) * (fv[:, 1, 0] - fv[:, 0, 0])
    l0, l1 = r64["pix_to_face"][..., 0], r64["pix_to_face"][..., 1]
    assert (area[l0[l0 >= 0]] > 0).all() and (area[l1[l1 >= 0]] < 0).all()


@pytest.mark.parametrize("persp", [False, True])
def test_culling_leaves_exactly_the_front_layer(persp):
    _, r64, _ = O.sphere_reference(2, 48, persp)
    _, c64, c32 = O.sphere_reference(2, 48, persp, True)
    cap_holds(c64, "culled sphere")
    assert (c64["pix_to_face"][..., 1:] == -1).all()
    assert (c64["pix_to_face"][..., 0] == r64["pix_to_face"][..., 0]).all()
    assert (c64["zbuf"][..., 0] == r64["zbuf"][..., 0]).all()
    assert (c64["pix_to_face"] == c32["pix_to_face"])[~c64["unsafe"]].all()


def test_the_cap_holds_on_the_other_scenes_of_the_gpu_tests():
    from iso_points_amd import cameras
    from iso_points_amd.ops import MeshRasterizer
    fv = O.stack_scene()
    for K in (1, 2, 3, 4, 5, 8):                              # dyadic: the float32 restatement agrees on EVERY pixel
        r64 = O.rasterize(fv, [0], [len(fv)], 32, K)
        r32 = O.rasterize(fv, [0], [len(fv)], 32, K, dtype=np.float32)
        assert (r64["pix_to_face"] == r32["pix_to_face"]).all()
        assert r64["pix_to_face"][0, 16, 16].tolist() == [10, 11, 9, 8, 7, 6, 5, 12][:K]
    fv = O.edge_scene()
    for S in (1, 15, 16, 17, 31, 50):
        r64 = O.rasterize(fv, [0], [len(fv)], S, 3)
        cap_holds(r64, "edges S = %d" % S)
        assert (r64["pix_to_face"][..., 1] >= 0).all() and not (r64["pix_to_face"] == 3).any()
    fv = O.skip_scene()
    r64 = O.rasterize(fv, [0], [len(fv)], 40, 4)
    cap_holds(r64, "skips")
    assert not np.isin(r64["pix_to_face"], (1, 2, 3)).any() and (r64["pix_to_face"] == 4).any()
    fv = O.heavy_tile_scene()
    r64 = O.rasterize(fv, [0], [len(fv)], 32, 4)
    cap_holds(r64, "heavy tile")
    assert (r64["pix_to_face"][0, :16, :16, 0] == len(fv) - 1).all()
    assert (r64["pix_to_face"][0, :16, :16, 3] >= 0).mean() > 0.5
    # no two of a pixel's five nearest float32 depths are equal, so no tie decides a slot: the reversed face list maps one to one
    r32 = O.rasterize(fv, [0], [len(fv)], 32, 5, dtype=np.float32)
    both = (r32["pix_to_face"][..., :-1] >= 0) & (r32["pix_to_face"][..., 1:] >= 0)
    assert (r32["zbuf"][..., :-1] < r32["zbuf"][..., 1:])[both].all()
    big, small = O.sphere_faces(2)[0], O.sphere_faces(0)[0]
    cap_holds(O.rasterize(np.concatenate([big, small]), [0, 320, 320], [320, 0, 20], 33, 3), "batch")
    v, f = O.icosphere(2)
    views = torch.stack([cameras.look_at_view(2.7, 20.0, 30.0), cameras.look_at_view(3.0, -10.0, 100.0),
                         cameras.look_at_view(2.5, 60.0, 250.0)])
    ndc, first, num, _ = MeshRasterizer((views, views @ cameras.perspective(60.0))).transform(
        (torch.from_numpy(v)[None], torch.from_numpy(f)[None]))
    cap_holds(O.rasterize(ndc.numpy(), first.tolist(), num.tolist(), 33, 2), "three cameras")
    cap_holds(O.rasterize(ndc[:320].numpy(), [0], [320], 48, 5), "render_views")


def test_one_axis_aligned_triangle_analytically():
    """Right triangle (0.5, -0.5), (-0.5, -0.5), (-0.5, 0.5) at S = 32: a centre (X, Y) = (odd / 32, odd / 32) is inside iff
    X > -0.5, Y > -0.5 and X + Y < 0.  Of the 16 x 16 centres in the square, 16 lie on the diagonal and half of the rest are
    inside: 120.  The centroid (-1/6, -1/6) is no pixel centre; the centre next to it, (-5/32, -5/32), has by hand: weight
    of the vertex (0.5, -0.5) X + 0.5 = 11/32, of (-0.5, 0.5) Y + 0.5 = 11/32, the third 10/32; the nearest outline is the
    hypotenuse X + Y = 0 at distance |X + Y| / sqrt(2)."""
    fv = np.array([[[0.5, -0.5, 2.0], [-0.5, -0.5, 4.0], [-0.5, 0.5, 8.0]]], dtype=np.float32)
    for dt in (np.float64, np.float32):
        r = O.rasterize(fv, [0], [1], 32, 2, dtype=dt)
        assert r["covered"].sum() == 120 and (r["pix_to_face"][..., 1] == -1).all()
        # unsafe by definition: the centres exactly on the hypotenuse's line, none of them covered
        assert r["unsafe"][0][np.arange(32), 31 - np.arange(32)].all() and not (r["unsafe"] & r["covered"]).any()
        c = (32 + 5 - 1) // 2                                 # 1 - (2c + 1) / 32 = -5/32
        assert abs(O.pixel_centres(32)[c] + 5.0 / 32.0) == 0
        assert r["pix_to_face"][0, c, c, 0] == 0
        assert np.allclose(r["bary"][0, c, c, 0], [11 / 32, 10 / 32, 11 / 32], atol=1e-7)
        assert np.isclose(r["zbuf"][0, c, c, 0], (11 * 2 + 10 * 4 + 11 * 8) / 32, atol=1e-6)
        assert np.isclose(r["dists"][0, c, c, 0], -((10 / 32) ** 2) / 2, atol=1e-7)
    p = O.rasterize(fv, [0], [1], 32, 1, perspective_correct=True)
    t = np.array([11 / 32 * 4 * 8, 10 / 32 * 2 * 8, 11 / 32 * 2 * 4])
    assert np.allclose(p["bary"][0, c, c, 0], t / t.sum(), atol=1e-12)
    # (0.5, -0.5) -> (-0.5, -0.5) -> (-0.5, 0.5) runs counter-clockwise in the displayed image (+X left): area > 0, kept;
    # the same face wound the other way is culled
    assert O.rasterize(fv, [0], [1], 32, 1, cull_backfaces=True)["covered"].sum() == 120
    assert O.rasterize(fv[:, ::-1].copy(), [0], [1], 32, 1, cull_backfaces=True)["covered"].sum() == 0
    assert O.rasterize(fv[:, ::-1].copy(), [0], [1], 32, 1)["covered"].sum() == 120


# ------------------------------------------------------------------------------------------------- shading, in plain torch
@pytest.mark.parametrize("light", [dict(), dict(light_direction=(0.3, 0.8, -0.5)), dict(light_location=(2.0, 2.0, 2.0))])
def test_hard_flat_shading_and_render_views_on_cpu_tensors(light):
    from iso_points_amd import cameras
    from iso_points_amd.mesh_raster import Fragments, hard_flat_shading, render_views
    _, r64, _ = O.sphere_reference(2, 48, False)
    _, world = O.sphere_faces(2)
    view = cameras.look_at_view(2.7, 20.0, 30.0)
    cam = np.linalg.inv(view.numpy().astype(np.float64))[3, :3]
    fr = Fragments(torch.from_numpy(r64["pix_to_face"]), torch.from_numpy(r64["zbuf"]), torch.from_numpy(r64["bary"]),
                   torch.from_numpy(r64["dists"]))
    colors = torch.rand(320, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for fc in (None, colors):
        want = O.flat_shading(r64["pix_to_face"][..., 0], r64["bary"][..., 0, :], world, cam,
                              face_colors=None if fc is None else fc.numpy(), background=(0.1, 0.2, 0.3), **light)
        img = hard_flat_shading(fr, torch.from_numpy(world).double(), torch.from_numpy(cam), face_colors=fc,
                                background=(0.1, 0.2, 0.3), **light)
        assert img.shape == (1, 48, 48, 4) and img.dtype == torch.float64
        assert np.abs(img.numpy() - want).max() < 1e-12
        covered = r64["covered"]
        assert (img.numpy()[..., 3] == covered).all() and np.allclose(img.numpy()[..., :3][~covered], (0.1, 0.2, 0.3))
        assert img.numpy()[..., :3][covered].min() >= 0.5 * (1.0 if fc is None else 0.0)      # ambient 0.5 on white texels
    out = render_views(None, (view[None], view[None] @ cameras.perspective(60.0)), zfar=50.0, fragments=fr,
                       face_verts_world=torch.from_numpy(world).double(), **light)
    want = O.flat_shading(r64["pix_to_face"][..., 0], r64["bary"][..., 0, :], world, cam, **light)
    assert np.abs(out.images.numpy() - want).max() < 1e-6                         # (the camera position from a float32 view matrix)
    assert out.mask.dtype == torch.uint8 and (out.mask.numpy()[..., 0] == 255 * r64["covered"]).all()
    assert (out.depth.numpy()[..., 0] == np.where(r64["covered"], r64["zbuf"][..., 0], 50.0)).all()
    with pytest.raises(ValueError):
        hard_flat_shading(fr, torch.from_numpy(world), torch.from_numpy(cam), light_direction=(0, 1, 0), light_location=(0, 1, 0))
