"""iso_points_amd.ops without a GPU: the two functions import, every argument error is raised before any GPU call, CPU
tensors are refused, the header, the ctypes table and the built library agree on the iso_mesh_* entries, the generator is
pinned by known answers (through iso_mesh_sample_draw, a host function that runs the kernel's own routine) and the numpy
oracle of tests/mesh_sample_oracle.py is checked against it and on its own statistics."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_sample_oracle as O

MESH_ENTRIES = ("iso_mesh_face_areas", "iso_mesh_sample_workspace_bytes", "iso_mesh_sample",
                "iso_mesh_sample_backward_workspace_bytes", "iso_mesh_sample_backward", "iso_mesh_sample_draw")

# counter words, key words -> output words (Philox4x32-10)
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def lib_draw(seed, mesh, sample):
    from iso_points_amd import _lib
    out = (ctypes.c_uint32 * 4)()
    assert _lib.load().iso_mesh_sample_draw(seed, mesh, sample, out) == 0
    return tuple(int(x) for x in out)


def signed64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def test_the_two_functions_import_without_a_gpu():
    from iso_points_amd import ops
    assert callable(ops.sample_points_from_meshes) and callable(ops.mesh_face_areas_normals)


def test_header_table_and_library_agree_on_the_mesh_entries():
    import test_abi
    from iso_points_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in MESH_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(s for s in declared if s.startswith("iso_mesh_")) == sorted(MESH_ENTRIES)
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("iso_mesh_")) == sorted(MESH_ENTRIES)
    txt = re.sub(r"/\*.*?\*/", "", open(test_abi.HEADER).read(), flags=re.S)
    for name in MESH_ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the section follows H and cites the call sites it serves
    head = open(test_abi.HEADER).read()
    assert head.index("H. Point-to-mesh face distances") < head.index("I. Sampling points on meshes")
    section = head.split("I. Sampling points on meshes")[1]
    for cite in ("evaluation.py:113", ":164", "scripts/create_mvr_data_from_mesh.py:171", "tests/test_projection.py:347"):
        assert cite in section, cite


def test_the_new_file_is_built_once_without_the_slp_vectoriser():
    import subprocess
    import test_abi
    root = os.path.dirname(os.path.dirname(test_abi.HEADER))
    out = subprocess.run(["make", "-n", "-B", "-C", root, "iso_points_amd/libisopoints_hip.so"], stdout=subprocess.PIPE,
                         text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and "mesh_sample.hip" in l]
    assert len(lines) == 1 and "-fno-slp-vectorize" in lines[0].split(), lines


def test_known_answers_of_the_generator():
    """The three vectors of the header's generator.  The numpy Philox takes all three; the library's draw fixes the last
    counter word at 0, so it takes the first as it stands and the other two with that word set to 0, against the numpy
    Philox (which the vectors have just pinned)."""
    for counter, key, want in KNOWN:
        got = O.philox4x32_10(counter, key)
        assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    assert lib_draw(0, 0, 0) == KNOWN[0][2]
    for counter, key, _ in KNOWN:
        seed = key[0] | (key[1] << 32)
        sample = counter[0] | (counter[1] << 32)
        mesh = counter[2]
        want = tuple(int(x) for x in O.philox4x32_10((counter[0], counter[1], mesh, 0), key))
        # the library takes the seed and the sample as int64 bit patterns and the mesh as a 32-bit one
        got = lib_draw(signed64(seed), mesh - (1 << 32) if mesh >= (1 << 31) else mesh, signed64(sample))
        assert got == want, (hex(seed), hex(mesh), hex(sample))
        assert tuple(int(x[0]) for x in O.draw_words(signed64(seed), mesh, np.array([sample], dtype=np.uint64))) == want
    # the third vector's mesh word is 0x13198a2e and its last counter word is NOT 0: the words differ from the vector
    assert lib_draw(signed64(0x299f31d0a4093822), 0x13198a2e, signed64(0x85a308d3243f6a88)) != KNOWN[2][2]


def test_numpy_oracle_equals_the_library_draw_on_1000_triples():
    rng = np.random.RandomState(3)
    seeds = [int(x) for x in rng.randint(0, 2 ** 62, 600, dtype=np.int64)] + [int(x) for x in rng.randint(0, 2 ** 31, 200)] \
        + [-1, -(2 ** 63), 2 ** 63 - 1, 2 ** 32, 2 ** 32 + 1] + [int(x) for x in -rng.randint(1, 2 ** 62, 195, dtype=np.int64)]
    assert len(seeds) == 1000 and sum(s > 2 ** 32 for s in seeds) > 500
    meshes = rng.randint(0, 70000, 1000)
    samples = np.concatenate([rng.randint(0, 2 ** 31, 900, dtype=np.int64), rng.randint(2 ** 32, 2 ** 40, 100, dtype=np.int64)])
    for seed, n, s in zip(seeds, meshes, samples):
        want = tuple(int(x[0]) for x in O.draw_words(seed, int(n), np.array([s])))
        assert lib_draw(seed, int(n), int(s)) == want, (seed, n, s)


def test_uniforms_are_exact_and_below_one():
    uf, u, v = O.uniforms(12345, 0, np.arange(5000))
    assert uf.dtype == np.float64 and u.dtype == np.float32 and v.dtype == np.float32
    assert (uf >= 0).all() and (uf < 1).all() and (u >= 0).all() and (u < 1).all() and (v >= 0).all() and (v < 1).all()
    assert ((uf * 2.0 ** 53) % 1 == 0).all() and ((u.astype(np.float64) * 2.0 ** 24) % 1 == 0).all()


def test_workspace_sizes_are_monotone_and_zero_sizes_legal():
    from iso_points_amd import _lib
    lib = _lib.load()
    sizes = [lib.iso_mesh_sample_workspace_bytes(n, t) for n, t in ((0, 0), (1, 0), (1, 1), (1, 2048), (1, 2049), (1, 80000),
                                                                    (3, 80000), (3, 1000000), (64, 1000000))]
    assert sizes[0] >= 0 and sizes == sorted(sizes), sizes
    assert lib.iso_mesh_sample_workspace_bytes(1, 80000) >= 80000 * 12
    back = [lib.iso_mesh_sample_backward_workspace_bytes(t, q) for t, q in ((0, 0), (1, 1), (1, 1000), (700, 1000), (700, 300000),
                                                                           (90000, 300000))]
    assert back[0] >= 0 and back == sorted(back), back
    assert lib.iso_mesh_sample_backward_workspace_bytes(500, 1000) >= 4 * (3 * 500 + 2 * 1000)
    # a call with nothing to do needs no device: it returns before it touches a pointer
    assert lib.iso_mesh_face_areas(None, 0, None, None, None) == 0
    assert lib.iso_mesh_sample(None, None, None, 0, 0, 0, 1, None, None, None, None, None, 0, None) == 0
    assert lib.iso_mesh_sample(None, None, None, 3, 100, 0, 1, None, None, None, None, None, 0, None) == 0
    assert lib.iso_mesh_sample(None, None, None, 0, 100, 10, 1, None, None, None, None, None, 0, None) == 0
    assert lib.iso_mesh_sample_backward(None, None, None, None, None, None, 0, 0, None, 0, None) == 0
    # bad sizes are an error, not a launch
    assert lib.iso_mesh_sample(None, None, None, 1, 10, -1, 1, None, None, None, None, None, 0, None) != 0
    assert lib.iso_mesh_sample(None, None, None, 1, 2 ** 31, 10, 1, None, None, None, None, None, 0, None) != 0
    assert lib.iso_mesh_sample(None, None, None, 2, 10, 2 ** 30, 1, None, None, None, None, None, 0, None) != 0
    assert lib.iso_mesh_face_areas(None, 2 ** 31, None, None, None) != 0
    assert lib.iso_mesh_sample_backward(None, None, None, None, None, None, 2 ** 31, 10, None, 0, None) != 0
    assert lib.iso_mesh_sample_backward(None, None, None, None, None, None, 10, -1, None, 0, None) != 0
    assert b"iso_mesh_sample" in lib.iso_last_error()


def mesh_tuple():
    return torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))


def test_bad_arguments_raise_value_error():
    from iso_points_amd.ops import mesh_face_areas_normals, sample_points_from_meshes
    verts, faces = mesh_tuple()
    for meshes in ((verts, faces.float()),                       # float faces in the tuple form
                   (verts, faces[:1]),                           # batch sizes
                   (verts[..., :2], faces),
                   (verts, faces[..., :2]),
                   (verts[0], faces[0]),
                   (verts, faces, torch.tensor([6, 7])),         # more faces than rows
                   (verts, faces, torch.tensor([6])),
                   (verts, faces, torch.tensor([-1, 3])),
                   (verts,),
                   object()):
        with pytest.raises(ValueError):
            sample_points_from_meshes(meshes, 10)
    with pytest.raises(ValueError):
        sample_points_from_meshes((verts, faces), -1)
    with pytest.raises(ValueError):
        sample_points_from_meshes((verts, faces), 2 ** 30)       # N * S = 2^31
    sample_limit_ok = 2 ** 30 - 1                                # N * S = 2^31 - 2: not a ValueError (refused as CPU input)
    with pytest.raises(RuntimeError, match="GPU"):
        sample_points_from_meshes((verts, faces), sample_limit_ok)
    for v, f in ((verts, faces[0]), (verts[0], faces[0].float()), (verts[0][:, :2], faces[0]), (verts[0], faces[0][:, :2])):
        with pytest.raises(ValueError):
            mesh_face_areas_normals(v, f)


def test_textures_are_not_implemented():
    from iso_points_amd.ops import sample_points_from_meshes
    with pytest.raises(NotImplementedError):
        sample_points_from_meshes(mesh_tuple(), 10, return_textures=True)


class StubMeshes(object):
    """What sample_points_from_meshes reads of a pytorch3d Meshes."""

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


def test_cpu_tensors_are_refused():
    from iso_points_amd.ops import mesh_face_areas_normals, sample_points_from_meshes
    verts, faces = mesh_tuple()
    for fn in (lambda: sample_points_from_meshes((verts, faces), 10),
               lambda: sample_points_from_meshes((verts, faces, torch.tensor([6, 2])), 10, return_normals=True),
               lambda: sample_points_from_meshes(StubMeshes(verts, faces), 10, return_faces=True),
               lambda: sample_points_from_meshes((verts, faces), 0),
               lambda: mesh_face_areas_normals(verts[0], faces[0])):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


def test_lengths_that_follow_from_the_shapes_are_never_read(monkeypatch):
    """No tensor is read on the way to the first GPU call (here: to the refusal of CPU tensors), the seed included."""
    from iso_points_amd.ops import sample_points_from_meshes

    def no_read(self):
        raise AssertionError("a tensor was read")
    monkeypatch.setattr(torch.Tensor, "tolist", no_read)
    monkeypatch.setattr(torch.Tensor, "item", no_read)
    verts, faces = mesh_tuple()
    with pytest.raises(RuntimeError, match="GPU"):
        sample_points_from_meshes((verts, faces), 100, return_normals=True)
    with pytest.raises(RuntimeError, match="GPU"):
        sample_points_from_meshes(StubMeshes(verts, faces), 100)


@pytest.mark.parametrize("k", [1, 2, 3, 12345])
def test_the_oracle_alone_passes_the_statistical_bounds_of_the_gpu_tests(k):
    """The scaled icosphere (320 faces), S = 200 000, at the seeds the GPU tests use (what a CPU generator seeded with 1, 2, 3
    and 12345 hands the call): chi-square of the face counts against S * area / A below 319 + 6 sqrt(638) = 471 and the
    three weight means within 5 sqrt(1/18 / S) = 2.6e-3 of 1/3.  Measured: chi-square 303 / 328 / 380 / 296, weight means
    within 1.3e-3 of 1/3."""
    S = 200000
    seed = O.seed_of(k)
    verts, faces = O.scaled_icosphere()
    tris = verts[faces]
    areas = O.face_areas32(tris)
    assert areas.max() / areas.min() > 3.0                       # the scaling made the areas differ
    d = O.sample(tris, seed, 0, S)
    chi2 = O.chi_square(d["face"], areas, S)
    means = d["bary"].astype(np.float64).mean(axis=0)
    print("seed %d: chi-square %.1f (bound %.1f), weight means - 1/3: %s (bound %.2e)" % (
        seed, chi2, O.CHI2_BOUND, means - 1.0 / 3.0, O.bary_mean_bound(S)))
    assert chi2 < O.CHI2_BOUND
    assert (np.abs(means - 1.0 / 3.0) <= O.bary_mean_bound(S)).all()
    assert (np.abs(d["bary"].astype(np.float64).sum(axis=1) - 1.0) < 3e-7).all()
    assert (d["margin"] > 0).all()


def test_the_oracle_never_chooses_a_face_without_area():
    verts, faces = O.scaled_icosphere()
    areas = O.face_areas32(verts[faces]).copy()
    areas[::16] = 0.0
    d = O.sample(verts[faces], 2, 0, 50000, areas=areas)
    assert (areas[d["face"]] > 0).all()
    assert (O.sample(verts[faces], 2, 0, 10, areas=np.zeros(320))["face"] == -1).all()
