"""The SIREN backward without a GPU: the tangent-form formulas of DESIGN.md 3.1c against the float64 oracle's double
backward, the iso_sirengrad_* entries of the C ABI (header, ctypes table, library, size helpers, iso_sirengrad_form at every
limit), the guard that the GPU cases reach every k_sirengrad_* kernel of the built library, and NormalLengthLoss."""
import re

import pytest
import torch

from siren_backward_oracle import make_net, make_points, seeded_UV, tangent_form_grads, torch_grads
from test_siren_backward_gpu import BACKWARD_CASES

ENTRIES = ["iso_sirengrad_backward", "iso_sirengrad_backward_b0", "iso_sirengrad_chunk_points", "iso_sirengrad_form",
           "iso_sirengrad_workspace_bytes", "iso_sirengrad_workspace_points"]


def _lib():
    from iso_points_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("L", [0, 1, 3])
@pytest.mark.parametrize("form", ["uv", "u_only", "v_only"])
def test_tangent_form_reproduces_the_double_backward(L, form):
    """One tangent column per point: the formulas the kernels implement give the oracle's double backward to 1e-12 of the
    largest entry, into every weight and bias and into the points; v = None is the first-order form."""
    net = make_net(16, L, seed=L).double()
    n = 37
    pts = make_points(n, seed=L + 1).double()
    U, V = (t.double() for t in seeded_UV(n, seed=L))
    if form == "u_only":
        V = None
    if form == "v_only":
        U = torch.zeros_like(U)
    want = torch_grads(net, pts, U, V, torch.float64)
    got = tangent_form_grads(net, pts, U, V)
    assert sorted(got) == sorted(want)
    for k in want:
        top = want[k].abs().max().item()
        assert got[k].shape == want[k].shape, k
        assert (got[k] - want[k]).abs().max().item() <= 1e-12 * max(top, 1.0), (k, top)
    assert want["points"].abs().max().item() > 0


def test_header_ctypes_table_and_library_agree_on_the_sirengrad_entries():
    import ctypes
    from iso_points_amd import _lib
    from test_abi import declared_symbols
    names = [s for s in declared_symbols() if s.startswith("iso_sirengrad_")]
    assert sorted(names) == ENTRIES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["iso_sirengrad_backward"][1]) == 15
    assert len(_lib.SIGNATURES["iso_sirengrad_backward_b0"][1]) == 16                  # + the tail of layer 0's bias


@pytest.mark.parametrize("shape", [(64, 0), (64, 1), (128, 3), (256, 3), (256, 8)])
def test_size_helpers_need_no_gpu_and_grow_with_n(shape):
    lib = _lib()
    H, L = shape
    raw = lib.iso_siren_raw_floats(H, L)
    chunk, ws_points = lib.iso_sirengrad_chunk_points(), lib.iso_sirengrad_workspace_points()
    assert chunk >= 64 and ws_points >= chunk and ws_points % chunk == 0
    last = 0
    for n in (0, 1, 7, 63, chunk, chunk + 1, 1500, ws_points, ws_points + 1, 262144):
        mw = min(max(n, 1), ws_points)
        want = 4 * (256 + 4 * (L + 1) * mw * H + (mw + chunk - 1) // chunk * raw)
        got = lib.iso_sirengrad_workspace_bytes(n, H, L)
        assert got == want and got >= last, n
        last = got
    assert lib.iso_sirengrad_workspace_bytes(ws_points + 1, H, L) == lib.iso_sirengrad_workspace_bytes(ws_points, H, L)
    # the widths and depths the entry point refuses have no size
    assert lib.iso_sirengrad_workspace_bytes(100, 48, L) == 0 and lib.iso_sirengrad_workspace_bytes(100, 512, L) == 0
    assert lib.iso_sirengrad_workspace_bytes(100, H, 9) == 0 and lib.iso_sirengrad_workspace_bytes(100, H, -1) == 0


def test_form_on_both_sides_of_every_limit():
    form = _lib().iso_sirengrad_form
    assert [form(H, 3) for H in (-1, 0, 1, 48, 64, 65, 128, 129, 200, 256, 257, 512)] == \
        [0, 0, 804, 804, 804, 808, 808, 816, 816, 816, 0, 0]
    assert [form(256, L) for L in (-1, 0, 1, 8, 9)] == [0, 816, 816, 816, 0]
    assert [form(64, L) for L in (-1, 0, 8, 9)] == [0, 804, 804, 0]


def test_gpu_cases_reach_every_sirengrad_kernel_of_the_library():
    """iso_sirengrad_form's code 800 + H / 16 names the instances k_sirengrad_sweep<H / 16, tangent>, tangent false being
    the first-order form (v absent); the GPU cases reach exactly the instances the code object holds.  The other kernels
    take the width as an argument.  A new kernel without a case fails here, on the CPU."""
    from test_abi import _code_object_kernels
    plain, inst = set(), set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_sirengrad_\w*)", name)
        if m:
            kernel, rest = m.group(2)[:int(m.group(1))], m.group(2)[int(m.group(1)):]
            t = re.match(r"ILi(\d+)ELb([01])EE", rest)
            (inst.add((kernel, int(t.group(1)), bool(int(t.group(2))))) if t else plain.add(kernel))
    assert plain == {"k_sirengrad_tn", "k_sirengrad_cols"}, sorted(plain)      # the reduce: csrc/grad_sums.hip, tests/test_grad_sums_cpu.py
    assert inst == {("k_sirengrad_sweep", nt, tan) for nt in (4, 8, 16) for tan in (False, True)}, sorted(inst)
    form = _lib().iso_sirengrad_form
    reached = {(form(H, L) - 800, tan) for H, L, tan in BACKWARD_CASES}
    assert reached == {(nt, tan) for _, nt, tan in inst}
    # the reverse GEMM and k_sirengrad_tn run only with a hidden layer: every width has such a case and one without
    for nt in (4, 8, 16):
        depths = {L for H, L, tan in BACKWARD_CASES if form(H, L) == 800 + nt}
        assert 0 in depths and max(depths) >= 3, (nt, depths)
    assert (64, 8, True) in BACKWARD_CASES
    assert {48, 200} <= {H for H, _, _ in BACKWARD_CASES}


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_normal_length_loss_is_the_reference_formula(reduction):
    from iso_points_amd.loss import NormalLengthLoss
    g = torch.Generator().manual_seed(3)
    normals = (torch.randn(5, 11, 3, generator=g) * 1.5).requires_grad_(True)
    loss = NormalLengthLoss(reduction=reduction)(normals)
    ref_in = normals.detach().clone().requires_grad_(True)
    ref = (ref_in.norm(p=2, dim=-1) - 1) ** 2                       # DSS/training/losses.py:82
    ref = ref.mean() if reduction == "mean" else (ref.sum() if reduction == "sum" else ref)
    assert loss.shape == ref.shape and torch.equal(loss, ref)
    w = torch.randn(ref.shape, generator=g)
    (loss * w).sum().backward()
    (ref * w).sum().backward()
    assert torch.equal(normals.grad, ref_in.grad)
    with pytest.raises(ValueError):
        NormalLengthLoss()(torch.zeros(4, 2))
    with pytest.raises(ValueError):
        NormalLengthLoss(reduction="median")
