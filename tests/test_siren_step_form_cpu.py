"""Build guard of the on-chip SIREN step kernels (siren_x3.hip, k_siren_step_x3_both_oc): they are in the library, hold
their whole state in registers and LDS, and fit the LDS of a gfx950 CU."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dynamic LDS of the launch (X3Shape<256, 4, 3, 2>): activations 16 K-steps x 3 tiles x 2 parts x 1 KiB, the exchange of
# the adjoint maxima 2 x 96 x 4 floats, the tile's points 96 x 16 B, the LDS part of the stash 4 waves x 7 groups x 2 KiB
DYN_LDS = 16 * 3 * 2 * 1024 + 2 * 96 * 4 * 4 + 96 * 16 + 4 * 7 * 2048
LDS_PER_CU = 163840


def test_on_chip_step_kernels_use_no_scratch_and_fit_lds():
    if not shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no ROCm llvm tools")
    from iso_points_amd import _lib
    spec = importlib.util.spec_from_file_location("spill_check", os.path.join(ROOT, "tools", "spill_check.py"))
    sc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sc)
    ks = sc.kernel_resources(_lib.LIB_PATH)
    assert DYN_LDS == 160256
    for L in (2, 3):
        # <H = 256, NB = 3, MINB = 1, CODED = false, LT = L>
        for pat in ("23k_siren_step_x3_both_ocILi256ELi3ELi1ELb0ELi%dE" % L,):
            hit = [k for k in ks if pat in k[0]]
            assert len(hit) == 1, (pat, hit)
            name, vgpr_spills, _, private, static_lds = hit[0]
            assert vgpr_spills == 0 and private == 0, hit[0]
            assert static_lds + DYN_LDS <= LDS_PER_CU, hit[0]
