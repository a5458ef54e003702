"""iso_points_amd.loss without a GPU: the module imports, every argument error is raised before any GPU call, CPU tensors
are refused, and the header, the ctypes table and the built library agree on the Chamfer entries."""
import ctypes

import pytest
import torch

CHAMFER_ENTRIES = ("iso_chamfer_nearest_workspace_bytes", "iso_chamfer_nearest", "iso_chamfer_backward_workspace_bytes",
                   "iso_chamfer_backward")


def clouds(N=2, P1=20, P2=15):
    g = torch.Generator().manual_seed(0)
    return torch.rand(N, P1, 3, generator=g), torch.rand(N, P2, 3, generator=g)


def test_module_imports_without_a_gpu():
    from iso_points_amd import loss
    assert callable(loss.chamfer_distance) and callable(loss.nearest_points)


@pytest.mark.parametrize("kw", [
    dict(batch_reduction="max"),
    dict(point_reduction="max"),
    dict(point_reduction=None),
    dict(x_lengths=torch.tensor([21, 20])),
    dict(y_lengths=torch.tensor([15, 16])),
    dict(x_lengths=torch.tensor([20])),
    dict(x_normals=torch.rand(2, 20, 3)),
    dict(y_normals=torch.rand(2, 15, 3)),
    dict(x_normals=torch.rand(2, 19, 3), y_normals=torch.rand(2, 15, 3)),
    dict(weights=torch.ones(3)),
    dict(weights=torch.tensor([1.0, -1.0])),
])
def test_bad_arguments_raise_value_error(kw):
    from iso_points_amd.loss import chamfer_distance
    x, y = clouds()
    with pytest.raises(ValueError):
        chamfer_distance(x, y, **kw)


def test_mismatched_batch_sizes_raise_value_error():
    from iso_points_amd.loss import chamfer_distance, nearest_points
    x, _ = clouds(N=2)
    _, y = clouds(N=3)
    with pytest.raises(ValueError):
        chamfer_distance(x, y)
    with pytest.raises(ValueError):
        nearest_points(x, y)
    with pytest.raises(ValueError):
        chamfer_distance(torch.rand(2, 20, 2), torch.rand(2, 15, 2))


def test_cpu_tensors_are_refused():
    from iso_points_amd.loss import chamfer_distance, nearest_points
    x, y = clouds()

    class PC(object):
        def points_padded(self):
            return x

        def num_points_per_cloud(self):
            return torch.tensor([20, 12])
    for fn in (lambda: chamfer_distance(x, y), lambda: nearest_points(x, y), lambda: chamfer_distance(PC(), y),
               lambda: chamfer_distance(x, y, x_normals=torch.rand(2, 20, 3), y_normals=torch.rand(2, 15, 3),
                                        weights=torch.ones(2), batch_reduction=None, point_reduction="sum")):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


def test_header_table_and_library_agree_on_the_chamfer_entries():
    import test_abi
    from iso_points_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in CHAMFER_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert sorted(s for s in declared if s.startswith("iso_chamfer")) == sorted(CHAMFER_ENTRIES)
    # the table's argument counts are the header's
    import os
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(test_abi.HEADER).read(), flags=re.S)
    for name in CHAMFER_ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert os.path.basename(test_abi.HEADER) == "isopoints.h"
    # each entry cites the call sites it serves
    section = open(test_abi.HEADER).read().split("G. Chamfer distance")[1]
    assert "evaluation.py:119" in section and "trainer.py:256" in section


def test_workspace_sizes_need_no_gpu():
    from iso_points_amd import _lib
    lib = _lib.load()
    assert lib.iso_chamfer_nearest_workspace_bytes(2, 1000, 500) >= 2 * 500 * 16
    assert lib.iso_chamfer_backward_workspace_bytes(2, 1000, 500) >= 4 * (3 * 2 * 1000 + 2 * 2 * 500)
    assert lib.iso_chamfer_nearest_workspace_bytes(0, 0, 0) >= 0
