"""Even sampling without a GPU: remove_close and sample_points_from_meshes_even import, every argument error is raised
before any GPU call, the header, the ctypes table and the built library agree on the iso_disk_* entries, and the numpy
oracle of tests/disk_oracle.py is checked on its own: the serial rule equals the parallel form, and on the sampler oracle's
draws it meets the conditions tests/test_even_sample_gpu.py imposes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import disk_oracle as D
import mesh_sample_oracle as M

DISK_ENTRIES = ("iso_disk_workspace_bytes", "iso_disk_begin", "iso_disk_rounds", "iso_disk_select", "iso_disk_area_radius")


def test_the_functions_import_without_a_gpu():
    from iso_points_amd import ops, point_processing
    assert callable(point_processing.remove_close) and callable(ops.sample_points_from_meshes_even)
    assert point_processing.ROUNDS_PER_BATCH == 16


def test_header_table_and_library_agree_on_the_disk_entries():
    import test_abi
    from iso_points_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in DISK_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(s for s in declared if s.startswith("iso_disk_")) == sorted(DISK_ENTRIES)
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("iso_disk_")) == sorted(DISK_ENTRIES)
    txt = re.sub(r"/\*.*?\*/", "", open(test_abi.HEADER).read(), flags=re.S)
    for name in DISK_ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_section_l_follows_k_and_cites_the_call_sites():
    import test_abi
    head = open(test_abi.HEADER).read()
    assert head.index("K. The point-cloud regularisers") < head.index("L. Even sampling: Poisson-disk elimination (csrc/disk.hip)")
    section = head.split("L. Even sampling: Poisson-disk elimination")[1]
    for cite in ("config.py:227", "DSS/training/trainer.py:255", "DSS/utils/dataset.py:123"):
        assert cite in section, cite


def test_the_new_file_is_built_once_without_the_slp_vectoriser():
    import subprocess
    import test_abi
    root = os.path.dirname(os.path.dirname(test_abi.HEADER))
    out = subprocess.run(["make", "-n", "-B", "-C", root, "iso_points_amd/libisopoints_hip.so"], stdout=subprocess.PIPE,
                         text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and "disk.hip" in l]
    assert len(lines) == 1 and "-fno-slp-vectorize" in lines[0].split(), lines


def test_workspace_sizes_and_calls_with_nothing_to_do_need_no_gpu():
    from iso_points_amd import _lib
    lib = _lib.load()
    sizes = [lib.iso_disk_workspace_bytes(n, p) for n, p in ((0, 0), (1, 0), (1, 1), (1, 2048), (1, 2049), (3, 2049),
                                                              (3, 3000000))]
    assert sizes[0] >= 0 and sizes == sorted(sizes), sizes
    assert lib.iso_disk_workspace_bytes(1, 1000) >= 1000 * 17
    assert lib.iso_disk_begin(None, None, None, None, 0, 100, None, 0, None) == 0
    assert lib.iso_disk_begin(None, None, None, None, 2, 0, None, 0, None) == 0
    assert lib.iso_disk_area_radius(None, None, None, 0, 0, 10, None, None) == 0
    # bad sizes are an error, not a launch
    assert lib.iso_disk_begin(None, None, None, None, -1, 100, None, 0, None) != 0
    assert lib.iso_disk_begin(None, None, None, None, 2, 2 ** 30, None, 0, None) != 0          # N * P = 2^31
    assert lib.iso_disk_begin(None, None, None, None, 1, 100, None, 0, None) != 0              # no workspace
    assert lib.iso_disk_rounds(None, None, None, None, 1, 100, 10, 0, 0, None, None, 0, None) != 0
    assert lib.iso_disk_select(1, 100, -1, None, None, None, None, 0, None) != 0
    assert lib.iso_disk_area_radius(None, None, None, 1, 10, 0, None, None) != 0
    assert b"iso_disk_" in lib.iso_last_error()


# ---------------------------------------------------------------------------------------------------------- the oracle
def both(points, r, **kw):
    conf = D.conflicts(points, r)
    ms, ss, ks = D.serial(points, r, conf=conf, **kw)
    mr, sr, kr, n = D.rounds(points, r, conf=conf, **kw)
    assert (ms == mr).all() and (ss == sr).all() and ks == kr
    # the definition's properties, checked on the result itself
    kept = np.nonzero(ms)[0]
    assert not np.triu(conf[np.ix_(kept, kept)], k=1).any()                       # no two kept samples conflict
    entry = D._entry_state(len(points), kw.get("length"), kw.get("valid")) == D.UNDECIDED
    for s in np.nonzero(entry & ~ms)[0]:                                          # a removed valid sample has a kept
        assert (conf[s, :s] & ms[:s]).any(), s                                    # conflicting sample below it
    assert not (ms & ~entry).any()
    return ms, ks, n


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_serial_equals_rounds_on_random_clouds(seed):
    rng = np.random.RandomState(seed)
    pts = D.sphere_cloud(900, seed)
    mask, kept, n = both(pts, 0.12)
    assert 0 < kept < 900 and n >= 2
    # prefix stability
    m2, _, _ = both(pts[:400], 0.12)
    assert (m2 == mask[:400]).all()
    # lengths and a validity mask
    valid = rng.rand(900) > 0.1
    m3, k3, _ = both(pts, 0.12, length=700, valid=valid)
    assert not m3[700:].any() and not (m3 & ~valid).any() and k3 > 0
    # a cube, another radius
    both(rng.rand(700, 3).astype(np.float32), 0.2)


def test_serial_equals_rounds_on_the_chain():
    r = 0.05
    pts, _ = D.chain(257, r)
    mask, kept, n = both(pts, r)
    assert (np.nonzero(mask)[0] == np.arange(0, 257, 2)).all() and kept == 129
    assert n == 257                                                               # one link per round
    pts, order = D.chain(257, r, shuffle_seed=4)
    mask, kept, n = both(pts, r)
    assert n < 257 and 86 <= kept <= 129      # between every third and every second position of the line


def test_serial_equals_rounds_with_duplicates_and_ties():
    rng = np.random.RandomState(5)
    base = rng.rand(200, 3).astype(np.float32)
    pts = np.concatenate([base, base[::2], base[:50]])
    mask, _, _ = both(pts, 1e-6)
    assert mask[:200].all() and not mask[200:].any()                              # the lower index of a duplicate is kept
    r = np.float32(0.3)
    far = np.nextafter(r, np.float32(1.0))
    pts = np.array([[0, 0, 0], [r, 0, 0], [5, 0, 0], [5, far, 0]], dtype=np.float32)
    mask, _, _ = both(pts, r)
    assert mask.tolist() == [True, False, True, True]                             # d2 == r2 conflicts, one ulp beyond does not


@pytest.mark.parametrize("name,S", D.SAMPLER_CASES)
def test_the_oracle_alone_meets_the_conditions_of_the_gpu_tests(name, S):
    """On the sampler oracle's 3 S draws at the seeds the GPU tests use and the default radius sqrt(A / (3 S)) the serial
    rule keeps at least S samples.  Measured: 335-345 of 300 on icosphere(2), 1130-1135 of 1000 on icosphere(3), 566-576 of
    500 on the scaled icosphere."""
    verts, faces = D.sampler_mesh(name)
    r = D.default_radius(verts, faces, S)
    for k in (1, 2, 3):
        pts, face = D.oracle_draw_points(verts, faces, M.seed_of(k), 3 * S)
        assert (face >= 0).all()
        conf = D.conflicts(pts, r)
        mask, sel, kept = D.serial(pts, r, conf=conf)
        print("%s S = %d seed %d: kept %d of %d draws at r = %.6f" % (name, S, k, kept, 3 * S, r))
        assert kept >= S
        _, _, kr, n = D.rounds(pts, r, conf=conf)
        assert kr == kept and n <= 16


# ------------------------------------------------------------------------------------------------------- bad arguments
def test_remove_close_bad_arguments_raise_value_error():
    from iso_points_amd.point_processing import remove_close
    x = torch.rand(2, 10, 3)
    for bad in (lambda: remove_close(x, 0.0),
                lambda: remove_close(x, -1.0),
                lambda: remove_close(x, float("nan")),
                lambda: remove_close(x, float("inf")),
                lambda: remove_close(x, "wide"),
                lambda: remove_close(x[0], 0.1),
                lambda: remove_close(x[..., :2], 0.1),
                lambda: remove_close(object(), 0.1),
                lambda: remove_close(x, torch.tensor([0.1])),                     # radius tensor of the wrong length
                lambda: remove_close(x, torch.rand(2, 1)),
                lambda: remove_close(x, 0.1, lengths=torch.tensor([10])),
                lambda: remove_close(x, 0.1, lengths=torch.tensor([10.0, 3.0])),
                lambda: remove_close(x, 0.1, lengths=torch.tensor([11, 3])),
                lambda: remove_close(x, 0.1, lengths=torch.tensor([-1, 3])),
                lambda: remove_close(x, 0.1, valid=torch.ones(2, 9)),
                lambda: remove_close(x, 0.1, valid=torch.ones(10))):
        with pytest.raises(ValueError):
            bad()


def test_cpu_tensors_are_refused():
    """remove_close lists CPU tensors among its ValueErrors and raises the package's RuntimeError at the same time."""
    from iso_points_amd.ops import sample_points_from_meshes_even
    from iso_points_amd.point_processing import remove_close
    x = torch.rand(2, 10, 3)
    for fn in (lambda: remove_close(x, 0.1),
               lambda: remove_close(x, torch.tensor([0.1, 0.2]), lengths=torch.tensor([10, 0]), valid=torch.ones(2, 10))):
        with pytest.raises(ValueError, match="GPU"):
            fn()
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))
    for fn in (lambda: sample_points_from_meshes_even((verts, faces), 10),
               lambda: sample_points_from_meshes_even((verts, faces), 10, 0.1, return_normals=True, return_faces=True),
               lambda: sample_points_from_meshes_even((verts, faces), 0)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


def test_even_sampler_bad_arguments_raise_value_error():
    from iso_points_amd.ops import sample_points_from_meshes_even
    verts, faces = torch.rand(2, 9, 3), torch.randint(0, 9, (2, 6, 3))
    for bad in (lambda: sample_points_from_meshes_even((verts, faces), -1),
                lambda: sample_points_from_meshes_even((verts, faces), 10, 0.0),
                lambda: sample_points_from_meshes_even((verts, faces), 10, float("nan")),
                lambda: sample_points_from_meshes_even((verts, faces), 10, float("inf")),
                lambda: sample_points_from_meshes_even((verts, faces), 10, torch.tensor([0.1])),
                lambda: sample_points_from_meshes_even((verts, faces), 10, oversample=0),
                lambda: sample_points_from_meshes_even((verts, faces.float()), 10),
                lambda: sample_points_from_meshes_even((verts,), 10),
                lambda: sample_points_from_meshes_even((verts, faces), 2 ** 30, oversample=1),      # N * S = 2^31
                lambda: sample_points_from_meshes_even((verts, faces), 2 ** 28, oversample=4)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU"):                                # N * 3 * S = 2^31 - 6: refused as CPU input
        sample_points_from_meshes_even((verts, faces), (2 ** 30 - 1) // 3)
