"""The point-to-face distances of iso_points_amd.loss without a GPU: the four functions import, every argument error is
raised before any GPU call, CPU tensors are refused, and the header, the ctypes table and the built library agree on the
iso_pfdist_* entries."""
import ctypes
import os
import re

import pytest
import torch

PFDIST_ENTRIES = ("iso_pfdist_prepare", "iso_pfdist_forward_workspace_bytes", "iso_pfdist_forward",
                  "iso_pfdist_backward_workspace_bytes", "iso_pfdist_backward")


def packed(P=(12, 8), T=(5, 7), seed=0):
    """Two clouds and two meshes, packed: points, points_first_idx, tris, tris_first_idx, max_points."""
    g = torch.Generator().manual_seed(seed)
    points, tris = torch.rand(sum(P), 3, generator=g), torch.rand(sum(T), 3, 3, generator=g)
    return points, torch.tensor([0, P[0]]), tris, torch.tensor([0, T[0]]), max(P)


def test_the_four_functions_import_without_a_gpu():
    from iso_points_amd import loss
    for name in ("point_face_distance", "face_point_distance", "point_mesh_face_distance", "nearest_faces"):
        assert callable(getattr(loss, name)), name


def test_header_table_and_library_agree_on_the_pfdist_entries():
    import test_abi
    from iso_points_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in PFDIST_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(s for s in declared if s.startswith("iso_pfdist")) == sorted(PFDIST_ENTRIES)
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("iso_pfdist")) == sorted(PFDIST_ENTRIES)
    # the table's argument counts are the header's
    txt = re.sub(r"/\*.*?\*/", "", open(test_abi.HEADER).read(), flags=re.S)
    for name in PFDIST_ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the section follows G and cites the call sites it serves
    head = open(test_abi.HEADER).read()
    assert head.index("G. Chamfer distance") < head.index("H. Point-to-mesh face distances")
    section = head.split("H. Point-to-mesh face distances")[1]
    assert "evaluation.py:78" in section and "losses.py:536-598" in section


def test_the_new_file_is_built_without_the_slp_vectoriser():
    import subprocess
    import test_abi
    root = os.path.dirname(os.path.dirname(test_abi.HEADER))
    out = subprocess.run(["make", "-n", "-B", "-C", root, "iso_points_amd/libisopoints_hip.so"], stdout=subprocess.PIPE,
                         text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and "pfdist.hip" in l]
    assert len(lines) == 1 and "-fno-slp-vectorize" in lines[0].split(), lines


def test_workspace_sizes_are_monotone_and_zero_sizes_legal():
    from iso_points_amd import _lib
    lib = _lib.load()
    for direction in (0, 1):
        rec = 48 if direction == 0 else 16
        assert lib.iso_pfdist_forward_workspace_bytes(direction, 2, 1000, 500) >= 2 * 500 * rec
        sizes = [lib.iso_pfdist_forward_workspace_bytes(direction, n, q, t)
                 for n, q, t in ((0, 0, 0), (1, 1, 1), (1, 1000, 1), (1, 1000, 700), (3, 1000, 700), (3, 300000, 700),
                                 (3, 300000, 90000))]
        assert sizes[0] >= 0 and sizes == sorted(sizes), sizes
        back = [lib.iso_pfdist_backward_workspace_bytes(direction, p, t)
                for p, t in ((0, 0), (1, 1), (1000, 1), (1000, 700), (300000, 700), (300000, 90000))]
        assert back[0] >= 0 and back == sorted(back), back
    assert lib.iso_pfdist_backward_workspace_bytes(0, 1000, 500) >= 4 * (3 * 500 + 2 * 1000)
    assert lib.iso_pfdist_backward_workspace_bytes(1, 1000, 500) >= 4 * (3 * 1000 + 2 * 500)
    # a call with nothing to do needs no device: it returns before it touches a pointer
    assert lib.iso_pfdist_prepare(None, None, None, None, None, None, 0, 0, 0, 0, 0, None, None, None, None, None) == 0
    assert lib.iso_pfdist_forward(0, None, None, None, None, None, None, None, None, None, None, None, None, None, 0.0,
                                  None, None, None, 0, 0, 0, 0, 0, 0, None, 0, None) == 0
    assert lib.iso_pfdist_backward(1, None, None, None, None, 0.0, None, None, 0, 0, None, 0, None) == 0
    # and a bad direction or a negative area is an error, not a launch
    assert lib.iso_pfdist_forward(2, None, None, None, None, None, None, None, None, None, None, None, None, None, 0.0,
                                  None, None, None, 0, 0, 0, 0, 0, 0, None, 0, None) != 0
    assert lib.iso_pfdist_forward(0, None, None, None, None, None, None, None, None, None, None, None, None, None, -1.0,
                                  None, None, None, 0, 0, 0, 0, 0, 0, None, 0, None) != 0


@pytest.mark.parametrize("change", [
    dict(points=torch.rand(20, 2)),
    dict(points=torch.rand(2, 10, 3)),
    dict(tris=torch.rand(12, 3)),
    dict(tris=torch.rand(12, 9)),
    dict(points_first_idx=torch.tensor([0, 12, 15])),          # three clouds, two meshes
    dict(points_first_idx=torch.tensor([[0, 12]])),
    dict(points_first_idx=torch.tensor([1, 12])),              # does not start at row 0
    dict(points_first_idx=torch.tensor([0, 21])),              # beyond the packed rows
    dict(tris_first_idx=torch.tensor([0, 13])),
    dict(tris_first_idx=torch.tensor([5, 0])),                 # descends
    dict(tris_first_idx=torch.tensor([0.0, 5.0])),
    dict(max_points=11),                                       # the first cloud holds 12
    dict(min_triangle_area=-1.0),
])
def test_bad_arguments_raise_value_error(change):
    from iso_points_amd.loss import face_point_distance, point_face_distance
    names = ("points", "points_first_idx", "tris", "tris_first_idx", "max_points")
    args = dict(zip(names, packed()))
    args.update(change)
    for fn in (point_face_distance, face_point_distance):
        with pytest.raises(ValueError):
            fn(*[args[k] for k in names], **({"min_triangle_area": args["min_triangle_area"]}
                                             if "min_triangle_area" in args else {}))


def test_bad_mesh_and_cloud_arguments_raise_value_error():
    from iso_points_amd.loss import nearest_faces, point_mesh_face_distance
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))
    pcl = torch.rand(2, 11, 3)
    for meshes, pcls in (((verts, faces), torch.rand(3, 11, 3)),                    # batch sizes
                         ((verts, faces), torch.rand(2, 11, 2)),
                         ((verts, faces.float()), pcl),
                         ((verts, faces[:1]), pcl),
                         ((verts[..., :2], faces), pcl),
                         ((verts, faces, torch.tensor([6, 7])), pcl),              # more faces than rows
                         ((verts, faces, torch.tensor([6])), pcl),
                         ((verts,), pcl),
                         (object(), pcl)):
        with pytest.raises(ValueError):
            point_mesh_face_distance(meshes, pcls)
    with pytest.raises(ValueError):
        point_mesh_face_distance((verts, faces), pcl, min_triangle_area=-1e-3)
    with pytest.raises(ValueError):
        nearest_faces(torch.rand(10, 3), torch.rand(4, 3, 3), points_first_idx=torch.tensor([0]))
    with pytest.raises(ValueError):
        nearest_faces(torch.rand(10, 2), torch.rand(4, 3, 3))


def test_cpu_tensors_are_refused():
    from iso_points_amd.loss import face_point_distance, nearest_faces, point_face_distance, point_mesh_face_distance
    args = packed()
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))

    class Mesh(object):
        def verts_packed(self):
            return verts.reshape(-1, 3)

        def faces_packed(self):
            return torch.cat([faces[0], faces[1] + 9])

        def mesh_to_faces_packed_first_idx(self):
            return torch.tensor([0, 6])

        def num_faces_per_mesh(self):
            return torch.tensor([6, 6])
    for fn in (lambda: point_face_distance(*args), lambda: face_point_distance(*args, min_triangle_area=5e-3),
               lambda: nearest_faces(args[0], args[2]), lambda: nearest_faces(args[0], args[2], args[1], args[3]),
               lambda: point_mesh_face_distance((verts, faces), torch.rand(2, 11, 3)),
               lambda: point_mesh_face_distance((verts, faces, torch.tensor([6, 2])), torch.rand(2, 11, 3)),
               lambda: point_mesh_face_distance(Mesh(), torch.rand(2, 11, 3), min_triangle_area=5e-3)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


def test_lengths_that_follow_from_the_shapes_are_never_read(monkeypatch):
    """The argument checks of point_mesh_face_distance use the host copies that shape-derived lengths carry: no tensor is
    read on the way to the first GPU call (here: to the refusal of CPU tensors)."""
    from iso_points_amd.loss import point_mesh_face_distance

    def no_read(self):
        raise AssertionError("a lengths tensor was read")
    monkeypatch.setattr(torch.Tensor, "tolist", no_read)
    monkeypatch.setattr(torch.Tensor, "item", no_read)
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        point_mesh_face_distance((verts, faces), torch.rand(2, 11, 3))
