"""The fused IDR SDF path without a GPU: the dispatch of iso_project_idr / iso_idr_sdf_grad / iso_trace_idr on both sides of
every boundary and in both GEMM modes (iso_idr_step_form), its refusals, the mode setter, and the guard that the cases of
tests/test_idr_forms_gpu.py reach every k_idr_step* kernel of the built library."""
import re

import pytest

from test_idr_forms_gpu import CASES, MODES

STAGED, FS, FS_VALUE, X16, X16_VALUE = 100, 200, 300, 400, 500


def _lib():
    from iso_points_amd import _lib
    return _lib.load()


@pytest.fixture
def mode():
    """Sets the IDR GEMM mode by name; the mode found is restored."""
    lib = _lib()
    before = lib.iso_idr_get_gemm_mode()

    def set_mode(name):
        assert lib.iso_idr_set_gemm_mode(MODES[name]) == 0
    yield set_mode
    assert lib.iso_idr_set_gemm_mode(before) == 0


def _expected(H, F, value_only, mode_name):
    """The table of include/isopoints.h, restated: D0 = 3 + 6 F."""
    NT, D0 = H // 16, 3 + 6 * F
    if mode_name == "split16" and H in (256, 512) and D0 <= 39:
        return (X16_VALUE if value_only else X16) + NT
    if D0 <= 48 and (value_only or H >= 256):
        return (FS_VALUE if value_only else FS) + NT
    return STAGED + NT


# (hidden, n_freq) on both sides of every boundary: F = 6 | 7 (split fp16 -> feature split), 7 | 8 (feature split ->
# staged), the ends 0 and 10, every width
BOUNDARY_SHAPES = [(H, F) for H in (128, 256, 512) for F in (0, 6, 7, 8, 10)]


@pytest.mark.parametrize("mode_name", ["split16", "f32"])
@pytest.mark.parametrize("value_only", [0, 1])
@pytest.mark.parametrize("H,F", BOUNDARY_SHAPES)
def test_dispatch_boundaries(mode, H, F, value_only, mode_name):
    lib = _lib()
    mode(mode_name)
    for NL, skip in ((2, -1), (3, 1), (8, 4), (12, 11)):
        assert lib.iso_idr_step_form(H, NL, skip, F, value_only) == _expected(H, F, value_only, mode_name), (NL, skip)


def test_dispatch_table_spelled_out(mode):
    """The same boundaries as literal codes, so that a mistake shared by _expected and the library cannot hide."""
    lib = _lib()

    def form(H, F, v):
        return lib.iso_idr_step_form(H, 4, 2, F, v)
    mode("split16")
    assert [form(512, F, 0) for F in (6, 7, 8)] == [432, 232, 132]
    assert [form(512, F, 1) for F in (6, 7, 8)] == [532, 332, 132]
    assert [form(256, F, 0) for F in (6, 7, 8)] == [416, 216, 116]
    assert [form(256, F, 1) for F in (6, 7, 8)] == [516, 316, 116]
    # H = 128: the staged kernel for the gradient, the feature-split one for the value while the encoding fits it
    assert [form(128, F, 0) for F in (0, 6, 7, 8, 10)] == [108] * 5
    assert [form(128, F, 1) for F in (0, 6, 7, 8, 10)] == [308, 308, 308, 108, 108]
    mode("f32")
    assert [form(512, F, 0) for F in (0, 6, 7, 8, 10)] == [232, 232, 232, 132, 132]
    assert [form(512, F, 1) for F in (0, 6, 7, 8, 10)] == [332, 332, 332, 132, 132]
    assert [form(256, F, 0) for F in (0, 6, 7, 8, 10)] == [216, 216, 216, 116, 116]
    assert [form(256, F, 1) for F in (0, 6, 7, 8, 10)] == [316, 316, 316, 116, 116]
    assert [form(128, F, 0) for F in (0, 7, 8, 10)] == [108] * 4
    assert [form(128, F, 1) for F in (0, 7, 8, 10)] == [308, 308, 108, 108]


@pytest.mark.parametrize("mode_name", ["split16", "f32"])
def test_dispatch_refuses_shapes_outside_the_contract(mode, mode_name):
    lib = _lib()
    mode(mode_name)
    for v in (0, 1):
        assert lib.iso_idr_step_form(256, 4, 2, 6, v) > 0
        for H in (64, 1024, 0, 384):
            assert lib.iso_idr_step_form(H, 4, 2, 6, v) == -1, H
        for NL in (1, 13, 0):
            assert lib.iso_idr_step_form(256, NL, -1, 6, v) == -1, NL
        for NL, skip in ((4, 0), (4, 4), (2, 2), (12, 12)):
            assert lib.iso_idr_step_form(256, NL, skip, 6, v) == -1, (NL, skip)
        for NL, skip in ((4, 1), (4, 3), (2, 1), (12, 11), (4, -1), (4, -5)):
            assert lib.iso_idr_step_form(256, NL, skip, 6, v) > 0, (NL, skip)
        assert lib.iso_idr_step_form(256, 4, 2, 11, v) == -1 and lib.iso_idr_step_form(256, 4, 2, -1, v) == -1
        assert lib.iso_idr_step_form(128, 4, 2, 10, v) == 108                     # D0 = 63 < 128: the widest encoding


def test_mode_setter():
    lib = _lib()
    before = lib.iso_idr_get_gemm_mode()
    assert before in (0, 1)
    try:
        for m in (0, 1, 0):
            assert lib.iso_idr_set_gemm_mode(m) == 0 and lib.iso_idr_get_gemm_mode() == m
            for bad in (2, -1, 7):
                assert lib.iso_idr_set_gemm_mode(bad) != 0
                assert b"iso_idr_set_gemm_mode" in lib.iso_last_error()
                assert lib.iso_idr_get_gemm_mode() == m                             # a refused value changes nothing
    finally:
        assert lib.iso_idr_set_gemm_mode(before) == 0
    assert lib.iso_idr_get_gemm_mode() == before
    # the IDR mode and the SIREN mode are two switches
    siren = lib.iso_siren_get_gemm_mode()
    try:
        assert lib.iso_idr_set_gemm_mode(1 - before) == 0
        assert lib.iso_siren_get_gemm_mode() == siren
        assert lib.iso_siren_set_gemm_mode(1 - siren) == 0
        assert lib.iso_idr_get_gemm_mode() == 1 - before
    finally:
        assert lib.iso_siren_set_gemm_mode(siren) == 0 and lib.iso_idr_set_gemm_mode(before) == 0


def _kernel_of(code, H):
    fam, NT = code // 100, code % 100
    assert NT == H // 16
    if fam == 1:
        return "k_idr_step<%d>" % NT
    if fam in (2, 3):
        return "k_idr_step_fs<%d,%d>" % (NT, fam == 3)
    return "k_idr_step_x16<%d,%d,%d>" % (H, {256: 3, 512: 2}[H], fam == 5)


def test_gpu_cases_reach_every_idr_step_kernel_of_the_library(mode):
    """The orphan guard: CASES (every shape, mode and value_only tests/test_idr_forms_gpu.py launches) taken through
    iso_idr_step_form reach exactly the k_idr_step* kernels the code object holds.  A re-dispatch that orphans an instance,
    or a new instance without a case, fails here, on the CPU.  k_idr_step_fs<8, false> is no kernel of the library: H = 128
    with the gradient is the staged kernel's."""
    from test_abi import _code_object_kernels
    in_library = set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_idr_step[a-z0-9_]*)I((?:L[ib]\d+E)+)E", name)
        if m and len(m.group(2)) == int(m.group(1)):
            in_library.add("%s<%s>" % (m.group(2), ",".join(re.findall(r"L[ib](\d+)E", m.group(3)))))
    lib = _lib()
    reached = set()
    for case, value_only in CASES:
        H, NL, skip, F, mode_name = case[:5]
        mode(mode_name)
        code = lib.iso_idr_step_form(H, NL, skip, F, value_only)
        assert code == case[5 + value_only], (case, value_only, code)
        reached.add(_kernel_of(code, H))
    print("reached: %s" % sorted(reached))
    assert len(in_library) == 12, sorted(in_library)
    assert "k_idr_step_fs<8,0>" not in in_library
    assert reached == in_library, (sorted(reached - in_library), sorted(in_library - reached))
