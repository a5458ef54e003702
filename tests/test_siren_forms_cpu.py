"""The fused SIREN SDF path without a GPU: the dispatch of iso_project_siren / iso_siren_sdf_grad / iso_trace_siren (and
their coded forms) on both sides of every boundary, in both GEMM modes and both step forms (iso_siren_step_kernel), its
refusals, the older queries that must follow the same table (iso_siren_step_form_used, iso_siren_step_launches), and the
guard that the table reaches exactly the k_siren_step* / k_siren_tail* kernels of the built library -- and that the cases of
tests/test_siren_forms_gpu.py do.  Nothing is launched."""
import itertools
import re

import pytest

from test_siren_forms_gpu import CASES, MODES, PROJECTED

F32, X3_VALUE, X3_128, BOTH, BOTH_OC = 100, 200, 300, 400, 500

WIDTHS, LAYERS = (64, 128, 256), (0, 1, 2, 3, 4, 8)
# (H, L, value_only, coded, GEMM mode, step form): every shape on both sides of every boundary, under every setting
GRID = list(itertools.product(WIDTHS, LAYERS, (0, 1), (0, 1), (0, 1), (0, 1)))


def _lib():
    from iso_points_amd import _lib
    return _lib.load()


def _tail_from_found(lib):
    """iso_siren_set_tail_from has no getter: the setting read back from iso_siren_step_launches (split-fp16 mode, a shape
    with a tail).  Default: 5 and 3 launches for T = 60 and 3; never: T + 1; k: k + 1 (k >= 60, the last iteration a
    projection may have, counts like never and reads as 0)."""
    t60, t3 = lib.iso_siren_step_launches(256, 1, 60), lib.iso_siren_step_launches(256, 1, 3)
    if (t60, t3) == (5, 3):
        return -1
    return 0 if t60 == 61 else t60 - 1


@pytest.fixture
def knobs():
    """Sets the GEMM mode, the step form and (optionally) tail_from; what was found is restored."""
    lib = _lib()
    mode, form = lib.iso_siren_get_gemm_mode(), lib.iso_siren_get_step_form()
    assert lib.iso_siren_set_gemm_mode(1) == 0
    tail = _tail_from_found(lib)
    assert lib.iso_siren_set_gemm_mode(mode) == 0

    def set_knobs(mode, form, tail_from=None):
        assert lib.iso_siren_set_gemm_mode(mode) == 0 and lib.iso_siren_set_step_form(form) == 0
        if tail_from is not None:
            assert lib.iso_siren_set_tail_from(tail_from) == 0
    yield set_knobs
    assert lib.iso_siren_set_gemm_mode(mode) == 0 and lib.iso_siren_set_step_form(form) == 0
    assert lib.iso_siren_set_tail_from(tail) == 0


def _expected(H, L, value_only, coded, mode, form):
    """The table of include/isopoints.h, restated."""
    NT = H // 16
    if mode == 0 or H == 64 or L == 0:
        return F32 + NT
    if value_only:
        return X3_VALUE + NT
    if H == 128:
        return X3_128 + NT
    if form == 1 and L in (2, 3) and not coded:
        return BOTH_OC + NT
    return BOTH + NT


def test_dispatch_boundaries(knobs):
    lib = _lib()
    for H, L, value_only, coded, mode, form in GRID:
        knobs(mode, form)
        assert lib.iso_siren_step_kernel(H, L, value_only, coded) == _expected(H, L, value_only, coded, mode, form), \
            (H, L, value_only, coded, mode, form)


def test_dispatch_table_spelled_out(knobs):
    """The same boundaries as literal codes, so that a mistake shared by _expected and the library cannot hide."""
    lib = _lib()

    def codes(H, value_only, coded, Ls=range(6)):
        return [lib.iso_siren_step_kernel(H, L, value_only, coded) for L in Ls]
    knobs(1, 1)
    assert codes(256, 0, 0) == [116, 416, 516, 516, 416, 416]
    assert codes(256, 0, 1) == [116, 416, 416, 416, 416, 416]
    assert codes(256, 1, 0) == codes(256, 1, 1) == [116, 216, 216, 216, 216, 216]
    assert codes(128, 0, 0) == codes(128, 0, 1) == [108, 308, 308, 308, 308, 308]
    assert codes(128, 1, 0) == codes(128, 1, 1) == [108, 208, 208, 208, 208, 208]
    assert codes(256, 0, 0, (7, 8)) == [416, 416] and codes(128, 0, 0, (8,)) == [308] and codes(128, 1, 1, (8,)) == [208]
    knobs(1, 0)
    assert codes(256, 0, 0) == codes(256, 0, 1) == [116, 416, 416, 416, 416, 416]
    assert codes(256, 1, 0) == [116, 216, 216, 216, 216, 216]
    assert codes(128, 0, 0) == [108, 308, 308, 308, 308, 308]
    for form in (0, 1):
        knobs(1, form)
        for v, c in itertools.product((0, 1), (0, 1)):
            assert codes(64, v, c, range(9)) == [104] * 9                         # H = 64: the f32 kernel in every mode
        knobs(0, form)
        for v, c in itertools.product((0, 1), (0, 1)):
            assert codes(64, v, c) == [104] * 6 and codes(128, v, c) == [108] * 6 and codes(256, v, c) == [116] * 6


@pytest.mark.parametrize("mode,form", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_dispatch_refuses_shapes_outside_the_contract(knobs, mode, form):
    lib = _lib()
    knobs(mode, form)
    for v, c in itertools.product((0, 1), (0, 1)):
        assert lib.iso_siren_step_kernel(256, 3, v, c) > 0
        for H in (0, 32, 96, 512):
            for L in (0, 1, 3, 8):
                assert lib.iso_siren_step_kernel(H, L, v, c) == -1, (H, L)
        for L in (-1, 9):
            for H in WIDTHS:
                assert lib.iso_siren_step_kernel(H, L, v, c) == -1, (H, L)


def test_step_form_used_is_the_gradient_steps_code(knobs):
    lib = _lib()
    for H, L, _, coded, mode, form in GRID:
        knobs(mode, form)
        assert lib.iso_siren_step_form_used(H, L, coded) == (lib.iso_siren_step_kernel(H, L, 0, coded) // 100 == 5), \
            (H, L, coded, mode, form)


def _launches(code, T, tail_from):
    """The tail rule restated: 4xx / 5xx run the iterations from `first` on as one launch."""
    if code // 100 not in (4, 5) or tail_from == 0:
        return T + 1
    first = tail_from if tail_from > 0 else (4 if T >= 6 else 2)
    return first + 1 if first <= T else T + 1


@pytest.mark.parametrize("tail_from", [-1, 0, 1, 7])
def test_step_launches_follow_the_tail_rule(knobs, tail_from):
    lib = _lib()
    for mode, form in itertools.product((0, 1), (0, 1)):
        knobs(mode, form, tail_from)
        for H, L in itertools.product(WIDTHS, LAYERS):
            code = lib.iso_siren_step_kernel(H, L, 0, 0)
            for T in range(13):
                assert lib.iso_siren_step_launches(H, L, T) == _launches(code, T, tail_from), (mode, form, H, L, T)
        assert lib.iso_siren_step_launches(256, 3, -1) == 0
    if tail_from == -1:                                                      # the values tests/test_siren_step_form_gpu.py asserts
        for form in (0, 1):
            knobs(1, form)
            assert lib.iso_siren_step_launches(256, 3, 10) == 5 and lib.iso_siren_step_launches(256, 3, 3) == 3
            assert lib.iso_siren_step_launches(128, 3, 10) == 11 and lib.iso_siren_step_launches(256, 0, 10) == 11
        knobs(0, 1)
        assert lib.iso_siren_step_launches(256, 3, 10) == 11


def test_fixture_reads_tail_from_back(knobs):
    lib = _lib()
    for k in (-1, 0, 1, 4, 7, 59):
        knobs(1, 1, k)
        assert _tail_from_found(lib) == k


def _kernel_of(code, H, L, coded):
    fam, NT = code // 100, code % 100
    assert NT == H // 16
    if fam == 1:
        return "k_siren_step<%d,%d>" % (NT, coded)
    if fam in (2, 3):
        assert (fam, H) != (3, 256)
        return "k_siren_step_x3<%s,%d,%d>" % ({128: "128,4,3,1", 256: "256,8,3,1"}[H], fam == 2, coded)
    if fam == 4:
        return "k_siren_step_x3_both<256,8,3,1,%d>" % coded
    assert fam == 5 and H == 256 and not coded
    return "k_siren_step_x3_both_oc<256,3,1,0,%d>" % L


TAIL_KERNELS = {"k_siren_tail_x3<256,8,1,0>", "k_siren_tail_x3<256,8,1,1>"}


def test_dispatch_reaches_every_siren_step_kernel_of_the_library(knobs):
    """The orphan guard: GRID taken through iso_siren_step_kernel reaches exactly the k_siren_step* kernels the code object
    holds, plus the two Newton-tail kernels (run for 4xx / 5xx, uncoded and coded).  A re-dispatch that orphans an
    instance, or a new instance that no code reaches, fails here, on the CPU.  The H = 256 gradient kernel of one tile
    shape and the one-shape on-chip kernel are no kernels of the library: every such call is a 416 / 516."""
    from test_abi import _code_object_kernels
    in_library = set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_siren_(?:step|tail)[a-z0-9_]*)I((?:L[ib]\d+E)+)E", name)
        if m and len(m.group(2)) == int(m.group(1)):
            in_library.add("%s<%s>" % (m.group(2), ",".join(re.findall(r"L[ib](\d+)E", m.group(3)))))
    lib = _lib()
    reached = set(TAIL_KERNELS)
    for H, L, value_only, coded, mode, form in GRID:
        knobs(mode, form)
        reached.add(_kernel_of(lib.iso_siren_step_kernel(H, L, value_only, coded), H, L, coded))
    print("reached: %s" % sorted(reached))
    assert len(in_library) == 18, sorted(in_library)
    assert not [k for k in in_library if k.startswith("k_siren_step_x3_oc<")]
    assert "k_siren_step_x3<256,8,3,1,0,0>" not in in_library and "k_siren_step_x3<256,8,3,1,0,1>" not in in_library
    assert reached == in_library, (sorted(reached - in_library), sorted(in_library - reached))


def _library_kernels():
    """The k_siren_step* / k_siren_tail* instances of the code object, as _kernel_of names them."""
    from test_abi import _code_object_kernels
    in_library = set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_siren_(?:step|tail)[a-z0-9_]*)I((?:L[ib]\d+E)+)E", name)
        if m and len(m.group(2)) == int(m.group(1)):
            in_library.add("%s<%s>" % (m.group(2), ",".join(re.findall(r"L[ib](\d+)E", m.group(3)))))
    return in_library


def test_gpu_cases_reach_every_siren_kernel_of_the_library(knobs):
    """The orphan guard on the GPU file: CASES (every shape, value_only, codedness, mode and step form that
    tests/test_siren_forms_gpu.py launches) taken through iso_siren_step_kernel give each case's expected code and reach
    exactly the 18 kernels the code object holds.  The two Newton-tail kernels count as reached only through a 4xx / 5xx
    gradient case of their codedness that the GPU file takes through a projection (PROJECTED).  A re-dispatch that orphans
    an instance, or a new instance without a case, fails here, on the CPU."""
    lib = _lib()
    in_library = _library_kernels()
    reached = set()
    for H, L, value_only, coded, mode, form, code in CASES:
        knobs(MODES[mode], form)
        assert lib.iso_siren_step_kernel(H, L, value_only, coded) == code, (H, L, value_only, coded, mode, form)
        reached.add(_kernel_of(code, H, L, coded))
    for H, L, coded, mode, form, code in PROJECTED:
        assert (H, L, 0, coded, mode, form, code) in CASES, (H, L, coded, mode, form, code)
        if code // 100 in (4, 5):
            assert H == 256
            reached.add("k_siren_tail_x3<256,8,1,%d>" % coded)
    print("reached: %s" % sorted(reached))
    assert TAIL_KERNELS <= reached, sorted(TAIL_KERNELS - reached)
    assert len(in_library) == 18, sorted(in_library)
    assert reached == in_library, (sorted(reached - in_library), sorted(in_library - reached))
