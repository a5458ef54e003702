"""The sign of the point-to-mesh distance (iso_points_amd.loss.mesh_pseudonormals / point_mesh_sign /
point_mesh_signed_distance) without a GPU: the three functions import, the header, the ctypes table and the built library
agree on the iso_pfsign_* entries, zero-size calls are legal, every argument error is raised before any GPU call, CPU
tensors are refused, the oracle of tests/pfsign_oracle.py agrees with the generalised winding number, and the kernels' own
per-pair routine (iso_pfsign_pair, a host function) agrees with the oracle on feature codes and weights."""
import ctypes
import os
import re

import pytest
import torch

import pfsign_oracle as O

PFSIGN_ENTRIES = ("iso_pfsign_normals_workspace_bytes", "iso_pfsign_normals", "iso_pfsign_sign", "iso_pfsign_pair")


def test_the_three_functions_import_without_a_gpu():
    from iso_points_amd import loss
    for name in ("mesh_pseudonormals", "point_mesh_sign", "point_mesh_signed_distance"):
        assert callable(getattr(loss, name)), name


def test_header_table_and_library_agree_on_the_pfsign_entries():
    import test_abi
    from iso_points_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in PFSIGN_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(s for s in declared if s.startswith("iso_pfsign")) == sorted(PFSIGN_ENTRIES)
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("iso_pfsign")) == sorted(PFSIGN_ENTRIES)
    txt = re.sub(r"/\*.*?\*/", "", open(test_abi.HEADER).read(), flags=re.S)
    for name in PFSIGN_ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the section follows I and cites the call site it serves
    head = open(test_abi.HEADER).read()
    assert head.index("I. Sampling points on meshes") < head.index("J. Sign of the point-to-mesh distance")
    assert "DSS/training/losses.py:536-598" in head.split("J. Sign of the point-to-mesh distance")[1]


def test_the_new_file_is_built_once_without_the_slp_vectoriser_and_pf_closest_has_one_definition():
    import subprocess
    import test_abi
    root = os.path.dirname(os.path.dirname(test_abi.HEADER))
    out = subprocess.run(["make", "-n", "-B", "-C", root, "iso_points_amd/libisopoints_hip.so"], stdout=subprocess.PIPE,
                         text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and "pfsign.hip" in l]
    assert len(lines) == 1 and "-fno-slp-vectorize" in lines[0].split(), lines
    csrc = os.path.join(root, "iso_points_amd", "csrc")
    defs = [n for n in sorted(os.listdir(csrc)) if re.search(r"float pf_closest\(", open(os.path.join(csrc, n)).read())]
    assert defs == ["pf_closest.h"], defs


def test_workspace_sizes_are_monotone_and_zero_sizes_legal():
    from iso_points_amd import _lib
    lib = _lib.load()
    sizes = [lib.iso_pfsign_normals_workspace_bytes(v, f) for v, f in ((0, 0), (1, 0), (1, 1), (128, 256), (1101, 1100),
                                                                       (40000, 80000), (40000, 800000), (400000, 800000))]
    assert sizes[0] >= 0 and sizes == sorted(sizes), sizes
    # two arrays over the corners and the gather's 3 V + 2 * 3 F ints
    assert lib.iso_pfsign_normals_workspace_bytes(500, 1000) >= 4 * (2 * 3000 + 3 * 500 + 2 * 3000)
    # a call with nothing to do needs no device: it returns before it touches a pointer
    assert lib.iso_pfsign_normals(None, None, 0, 0, None, None, None, None, 0, None) == 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, 0, 0, 0, None) == 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, 0, 100, 50, None) == 0
    # bad sizes are an error, not a launch
    assert lib.iso_pfsign_normals(None, None, -1, 0, None, None, None, None, 0, None) != 0
    assert lib.iso_pfsign_normals(None, None, 2 ** 31, 10, None, None, None, None, 0, None) != 0
    assert lib.iso_pfsign_normals(None, None, 10, (2 ** 31) // 3 + 1, None, None, None, None, 0, None) != 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, -1, 0, 0, None) != 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, 2 ** 31, 0, 0, None) != 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, 10, 2 ** 31, 0, None) != 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, -1.0, None, None, 0, 0, 0, None) != 0
    assert b"iso_pfsign_sign" in lib.iso_last_error()
    assert lib.iso_pfsign_pair(None, None, 0.0, None, None, None) != 0


# ---------------------------------------------------------------------------------------------------------- arguments
def mesh_tuple():
    return torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))


class StubMeshes(object):
    """What the sign reads of a pytorch3d Meshes."""

    def __init__(self, verts, faces):
        self.v, self.f = verts, faces

    def verts_packed(self):
        return self.v.reshape(-1, 3)

    def faces_packed(self):
        V = self.v.shape[1]
        return torch.cat([self.f[n] + n * V for n in range(self.f.shape[0])])

    def mesh_to_faces_packed_first_idx(self):
        return torch.arange(self.f.shape[0]) * self.f.shape[1]

    def num_faces_per_mesh(self):
        return torch.full((self.f.shape[0],), self.f.shape[1])


def test_bad_arguments_raise_value_error():
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign, point_mesh_signed_distance
    verts, faces = mesh_tuple()
    pcl = torch.rand(2, 11, 3)
    bad_meshes = ((verts, faces.float()), (verts, faces[:1]), (verts[..., :2], faces), (verts, faces[..., :2]),
                  (verts[0], faces[0]), (verts, faces, torch.tensor([6, 7])), (verts, faces, torch.tensor([6])),
                  (verts, faces, torch.tensor([-1, 3])), (verts,), object())
    for meshes in bad_meshes:
        with pytest.raises(ValueError):
            mesh_pseudonormals(meshes)
        for fn in (point_mesh_sign, point_mesh_signed_distance):
            with pytest.raises(ValueError):
                fn(meshes, pcl)
    one = (verts[:1], faces[:1])
    good_normals = (torch.rand(6, 3), torch.rand(6, 3, 3), torch.rand(9, 3))
    for fn in (point_mesh_sign, point_mesh_signed_distance):
        for meshes, pcls in (((verts, faces), torch.rand(3, 11, 3)),          # batch sizes
                             ((verts, faces), torch.rand(2, 11, 2)),
                             ((verts, faces), torch.rand(11, 3)),              # a flat cloud needs ONE mesh
                             (one, torch.rand(11, 2)),
                             (one, torch.rand(11)),
                             (one, "points")):
            with pytest.raises(ValueError):
                fn(meshes, pcls)
        with pytest.raises(ValueError):
            fn((verts, faces), pcl, min_triangle_area=-1e-3)
        for normals in (good_normals[:2], good_normals[0], (good_normals[0], good_normals[1], torch.rand(8, 3)),
                        (torch.rand(6, 3), torch.rand(6, 9), torch.rand(9, 3)),
                        (good_normals[0], good_normals[1], torch.zeros(9, 3, dtype=torch.int64)),
                        (torch.rand(5, 3), good_normals[1], good_normals[2])):
            with pytest.raises(ValueError):
                fn(one, torch.rand(11, 3), normals=normals)


def test_cpu_tensors_are_refused():
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign, point_mesh_signed_distance
    verts, faces = mesh_tuple()
    one = (verts[:1], faces[:1])
    normals = (torch.rand(6, 3), torch.rand(6, 3, 3), torch.rand(9, 3))
    for fn in (lambda: mesh_pseudonormals((verts, faces)),
               lambda: mesh_pseudonormals((verts, faces, torch.tensor([6, 2]))),
               lambda: mesh_pseudonormals(StubMeshes(verts, faces)),
               lambda: point_mesh_sign((verts, faces), torch.rand(2, 11, 3)),
               lambda: point_mesh_sign(one, torch.rand(11, 3), return_parts=True),
               lambda: point_mesh_sign(one, torch.rand(11, 3), normals=normals),
               lambda: point_mesh_sign(StubMeshes(verts, faces), torch.rand(2, 11, 3), min_triangle_area=5e-3),
               lambda: point_mesh_signed_distance((verts, faces, torch.tensor([6, 2])), torch.rand(2, 11, 3)),
               lambda: point_mesh_signed_distance(one, torch.rand(11, 3), normals=normals)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


def test_lengths_that_follow_from_the_shapes_are_never_read(monkeypatch):
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign, point_mesh_signed_distance

    def no_read(self):
        raise AssertionError("a tensor was read")
    monkeypatch.setattr(torch.Tensor, "tolist", no_read)
    monkeypatch.setattr(torch.Tensor, "item", no_read)
    verts, faces = mesh_tuple()
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_pseudonormals((verts, faces))
    with pytest.raises(RuntimeError, match="GPU"):
        point_mesh_sign((verts, faces), torch.rand(2, 11, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        point_mesh_signed_distance((verts[:1], faces[:1]), torch.rand(11, 3))


def test_packed_indices_of_both_mesh_forms():
    """The tuple form's local indices get n * V added, with and without num_faces, and equal the Meshes form's."""
    from iso_points_amd import loss
    verts, faces = mesh_tuple()
    v1, f1, t1, first1 = loss._packed_mesh_indexed((verts, faces), "test")
    v2, f2, t2, first2 = loss._packed_mesh_indexed(StubMeshes(verts, faces), "test")
    assert f1.dtype == torch.int64 and torch.equal(f1, f2) and torch.equal(v1, v2) and torch.equal(t1, t2)
    assert torch.equal(v1[f1], t1) and torch.equal(first1, first2)
    v3, f3, t3, first3 = loss._packed_mesh_indexed((verts, faces, torch.tensor([6, 2])), "test")
    assert f3.shape == (8, 3) and torch.equal(f3[6:], faces[1, :2] + 9) and torch.equal(v3[f3], t3)
    assert first3.tolist() == [0, 6]


# ---------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", ["torus", "cube"])
def test_the_oracle_agrees_with_the_winding_number(name):
    """The float64 pseudonormal rule against the generalised winding number on every point of the test sets (measured: 0
    mismatches of 6128 / 6008, the winding numbers within 1e-14 of 0 or 1); face, edge and vertex features all occur; and
    the same rule in float32 gives the same sign on every point."""
    verts, faces, points, ref = O.case(name)
    assert points.shape[0] == 6000 + verts.shape[0]
    want, w = O.winding_sign(points, verts, faces)
    assert ((w - w.round()).abs() < 1e-9).all()                       # a closed mesh: the number is an integer
    assert int((want != ref["sign"]).sum()) == 0
    assert (ref["sign"] < 0).sum() > 1000 and (ref["sign"] > 0).sum() > 1000
    counts = torch.bincount(ref["feature"].long(), minlength=7)
    print(name, "features", counts.tolist(), "min distance %.3g" % ref["dist"].min().item())
    assert (counts > 0).all()
    f32 = O.signed(points, verts, faces)
    assert int((f32["sign"].double() != ref["sign"]).sum()) == 0
    assert torch.equal(f32["idx"][ref["clear"]], ref["idx"][ref["clear"]])
    assert torch.equal(f32["feature"][ref["clear"]], ref["feature"][ref["clear"]])


def test_the_plain_face_normal_rule_fails_on_a_tetrahedron():
    """Why pseudonormals: beyond an edge, close to one face's normal, the OTHER face of the edge sees the point behind it."""
    verts, faces = O.tetrahedron()
    fn, en, vn = O.pseudonormals(verts.double(), faces)
    assert abs(O.dot3(fn[0], fn[1]).item() + 1.0 / 3.0) < 1e-12
    mid = 0.5 * (verts[0] + verts[1]).double()                         # the edge faces 0 and 1 share
    p = (mid + 0.3 * (0.8 * fn[0] + 0.2 * fn[1]))[None]              # inside the edge's wedge, near face 0's normal
    assert O.dot3(p - mid, fn[1]).item() < 0                           # the plain rule with face 1: inside
    ref = O.signed(p, verts.double(), faces)
    assert ref["sign"].item() == 1.0 and O.winding_sign(p, verts, faces)[0].item() == 1.0
    assert ref["feature"].item() in (1, 2, 3)


# ------------------------------------------------------------------------------------------------- the host pair routine
def lib_pair(p, tri, min_area=0.0):
    from iso_points_amd import _lib
    pa = (ctypes.c_float * 3)(*[float(x) for x in p])
    ta = (ctypes.c_float * 9)(*[float(x) for x in tri.reshape(-1)])
    d2, bw, feat = ctypes.c_float(), (ctypes.c_float * 3)(), ctypes.c_int32()
    assert _lib.load().iso_pfsign_pair(pa, ta, min_area, ctypes.byref(d2), bw, ctypes.byref(feat)) == 0
    return d2.value, [bw[0], bw[1], bw[2]], feat.value


def tetrahedron_probes(dist=0.3, jitter=0.01, seed=5):
    """Points beyond each of the tetrahedron's 4 faces, 6 edges and 4 vertices along that feature's pseudonormal, moved a
    little sideways so that no point sits on a plane of symmetry; with the feature as (kind, vertex set)."""
    verts, faces = O.tetrahedron()
    fn, en, vn = O.pseudonormals(verts.double(), faces)
    g = torch.Generator().manual_seed(seed)
    out = []
    for f in range(4):
        out.append((verts[faces[f]].double().mean(dim=0) + dist * fn[f], ("face", frozenset(faces[f].tolist()))))
        for k in range(3):
            a, b = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            if a < b:
                N = en[f, k] / en[f, k].norm()
                out.append((0.5 * (verts[a] + verts[b]).double() + dist * N, ("edge", frozenset((a, b)))))
    for v in range(4):
        out.append((verts[v].double() + dist * vn[v] / vn[v].norm(), ("vertex", frozenset((v,)))))
    pts = torch.stack([p for p, _ in out]) + jitter * (torch.rand(len(out), 3, generator=g, dtype=torch.float64) - 0.5)
    return verts, faces, pts.float(), [k for _, k in out]


def feature_vertices(face, code):
    if code == 0:
        return ("face", frozenset(face))
    if code <= 3:
        return ("edge", frozenset((face[code - 1], face[code % 3])))
    return ("vertex", frozenset((face[code - 4],)))


def test_host_pair_routine_on_a_vertex_an_edge_and_in_a_face():
    """Coordinates with few bits: the closest point is the point itself, d2 == 0, and the weights are exact."""
    tri = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    for p, code, bw in (((0.0, 0.0, 0.0), 4, [1.0, 0.0, 0.0]), ((1.0, 0.0, 0.0), 5, [0.0, 1.0, 0.0]),
                        ((0.0, 1.0, 0.0), 6, [0.0, 0.0, 1.0]), ((0.5, 0.0, 0.0), 1, [0.5, 0.5, 0.0]),
                        ((0.5, 0.5, 0.0), 2, [0.0, 0.5, 0.5]), ((0.0, 0.25, 0.0), 3, [0.75, 0.0, 0.25]),
                        ((0.25, 0.25, 0.0), 0, [0.5, 0.25, 0.25])):
        d2, got, feat = lib_pair(p, tri)
        assert d2 == 0.0 and got == bw and feat == code, (p, d2, got, feat)
        want = O.feature_of(O.pair_closest(torch.tensor(p, dtype=torch.float64), tri.double())[1])
        assert int(want) == code
    # above the same spots the feature stays; a face without area is measured by its edges and gives no NaN
    assert lib_pair((0.25, 0.25, 2.0), tri)[2] == 0 and lib_pair((-1.0, -1.0, 2.0), tri)[2] == 4
    assert lib_pair((0.25, 0.25, 2.0), tri, min_area=1.0)[2] != 0     # area 0.5 <= 1.0: the edges only
    flat = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    d2, bw, feat = lib_pair((0.5, 1.0, 0.0), flat)
    assert d2 == 1.0 and feat in (2, 3) and bw in ([0.0, 0.5, 0.5], [0.5, 0.0, 0.5])


def test_host_pair_routine_against_the_oracle_on_a_tetrahedron():
    """Every probe against every face of the tetrahedron (14 x 4 pairs): the feature code equals the float64 oracle's, the
    probe's own feature is found on every face that holds it, and the weights and d2 are within the float32 error of the
    formula: 4 x the largest error of the same formula in torch float32 against float64 on these very pairs."""
    verts, faces, pts, kinds = tetrahedron_probes()
    tri = verts[faces]
    d64, w64 = O.pair_closest(pts.double()[:, None, :], tri.double()[None])
    d32, w32 = O.pair_closest(pts[:, None, :], tri[None])
    A_w = 4.0 * (w32.double() - w64).abs().max().item()
    A_d = 4.0 * (d32.double() - d64).abs().max().item()
    print("A weights %.3g, d2 %.3g" % (A_w, A_d))
    assert 0 < A_w < 1e-5 and 0 < A_d < 1e-5
    want = O.feature_of(w64)
    seen = set()
    for i in range(pts.shape[0]):
        for f in range(4):
            d2, bw, feat = lib_pair(pts[i], tri[f])
            assert feat == int(want[i, f]), (i, f, feat, int(want[i, f]))
            assert abs(d2 - d64[i, f].item()) <= A_d
            assert max(abs(bw[k] - w64[i, f, k].item()) for k in range(3)) <= A_w
            if kinds[i][1] <= frozenset(faces[f].tolist()):
                assert feature_vertices(faces[f].tolist(), feat) == kinds[i], (i, f, feat, kinds[i])
                seen.add(feat)
    assert seen == set(range(7)), seen


def test_the_size_limits_are_the_librarys_own():
    """What the library would refuse is a ValueError before any GPU work, by the same inequalities (meta tensors: shapes
    without memory)."""
    from iso_points_amd import _lib
    from iso_points_amd.loss import mesh_pseudonormals, point_mesh_sign
    lib = _lib.load()

    class Meta(object):
        def __init__(self, V, F):
            self.V, self.F = V, F

        def verts_packed(self):
            return torch.empty((self.V, 3), device="meta")

        def faces_packed(self):
            return torch.empty((self.F, 3), dtype=torch.int64, device="meta")

        def mesh_to_faces_packed_first_idx(self):
            return torch.zeros(1, dtype=torch.int64)

        def num_faces_per_mesh(self):
            return torch.tensor([self.F])
    edge = (2 ** 31 - 1) // 3                                           # 715827882: the first face count refused
    assert lib.iso_pfsign_normals(None, None, 10, edge, None, None, None, None, 0, None) != 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, 0, edge, 10, None) != 0
    assert lib.iso_pfsign_sign(None, None, None, None, None, None, None, 0.0, None, None, 0, edge - 1, 10, None) == 0
    for V, F in ((10, edge), (2 ** 31 - 1, 4)):
        with pytest.raises(ValueError):
            mesh_pseudonormals(Meta(V, F))
        with pytest.raises(ValueError):
            point_mesh_sign(Meta(V, F), torch.rand(11, 3))
    with pytest.raises(RuntimeError, match="GPU"):                      # one below the limit: not a ValueError
        mesh_pseudonormals(Meta(10, edge - 1))
