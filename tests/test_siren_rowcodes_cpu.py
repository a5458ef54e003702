"""The SIREN backward with one latent code per cloud, without a GPU: the iso_sirencode_* entries of the C ABI (header, ctypes
table, library, size helper), the guard that the GPU cases reach every new kernel of the built library, the formulas of
DESIGN.md 3.1c ("One code per cloud") against float64 autograd, the wrapper's ordering helper and its argument errors."""
import re

import pytest
import torch

from siren_backward_oracle import make_net, make_points, seeded_UV
from siren_rowcodes_oracle import make_table, rows_from_lengths, table_form_grads, table_grads
from test_siren_rowcodes_gpu import EDGE_LENGTHS, ROWCODE_CASES

ENTRIES = ["iso_sirencode_backward", "iso_sirencode_workspace_bytes"]


def _lib():
    from iso_points_amd import _lib
    return _lib.load()


def test_header_ctypes_table_and_library_agree_on_the_sirencode_entries():
    import ctypes
    from iso_points_amd import _lib
    from test_abi import declared_symbols
    names = [s for s in declared_symbols() if s.startswith("iso_sirencode_")]
    assert sorted(names) == ENTRIES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["iso_sirencode_workspace_bytes"][1]) == 4
    # iso_sirengrad_backward_b0's without raw and b0_tail, + table, tail, code_of, code_first, n_codes, + the table's gradient
    assert len(_lib.SIGNATURES["iso_sirencode_backward"][1]) == 16 - 2 + 5 + 1
    assert _lib.SIGNATURES["iso_sirencode_backward"][1][13] is ctypes.c_int64              # n_codes


@pytest.mark.parametrize("shape", [(64, 0), (64, 1), (128, 3), (256, 3), (256, 8)])
def test_size_helper_needs_no_gpu(shape):
    """the uncoded size plus two partial rows of `hidden` floats per 256-point piece of a workspace chunk; it grows with n
    up to the workspace chunk, never shrinks with n_codes (the partials are per piece, not per code), 0 when refused"""
    lib = _lib()
    H, L = shape
    chunk, ws_points = lib.iso_sirengrad_chunk_points(), lib.iso_sirengrad_workspace_points()
    last = 0
    for n in (0, 1, 7, 63, chunk, chunk + 1, 1500, ws_points, ws_points + 1, 262144):
        mw = min(max(n, 1), ws_points)
        sizes = [lib.iso_sirencode_workspace_bytes(n, H, L, U) for U in (1, 2, 64, 100000)]
        assert sizes[0] == lib.iso_sirengrad_workspace_bytes(n, H, L) + 4 * 2 * H * ((mw + chunk - 1) // chunk), n
        assert sizes == sorted(sizes) and sizes[0] >= last, n
        if n in (chunk + 1, 1500, ws_points):
            assert sizes[0] > last, n
        last = sizes[0]
    for U in (0, -1):
        assert lib.iso_sirencode_workspace_bytes(100, H, L, U) == 0
    assert lib.iso_sirencode_workspace_bytes(100, 48, L, 2) == 0 and lib.iso_sirencode_workspace_bytes(100, 512, L, 2) == 0
    assert lib.iso_sirencode_workspace_bytes(100, H, 9, 2) == 0 and lib.iso_sirencode_workspace_bytes(100, H, -1, 2) == 0


def test_gpu_cases_reach_every_sirencode_kernel_of_the_library():
    """The new kernels take the width as an argument: k_sirencode_rows and k_sirencode_join run whenever the table's gradient
    is asked for.  The coded sweep is a run-time branch of k_sirengrad_sweep<H / 16, tangent>: the GPU cases of
    tests/test_siren_rowcodes_gpu.py reach every instance the code object holds, with and without a hidden layer, and the
    rows' boundary cases in both forms.  A new kernel without a case fails here, on the CPU."""
    from test_abi import _code_object_kernels
    plain, inst = set(), set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_sirencode_\w*)", name)
        if m:
            plain.add(m.group(2)[:int(m.group(1))])
            assert len(m.group(2)) - int(m.group(1)) <= len("ENS_6ScArgsE"), name          # no template instance
        m = re.search(r"_GLOBAL__N_1(\d+)(k_sirengrad_sweep\w*)", name)
        if m:
            t = re.match(r"ILi(\d+)ELb([01])EE", m.group(2)[int(m.group(1)):])
            inst.add((int(t.group(1)), bool(int(t.group(2)))))
    assert plain == {"k_sirencode_rows", "k_sirencode_join"}, sorted(plain)
    form = _lib().iso_sirengrad_form
    assert {(form(H, L) - 800, tan) for H, L, tan in ROWCODE_CASES} == inst
    for nt, tan in inst:
        depths = {L for H, L, t in ROWCODE_CASES if form(H, L) == 800 + nt and t == tan}
        assert 0 in depths and max(depths) >= 3, (nt, tan, depths)
    assert {48, 200} <= {H for H, _, _ in ROWCODE_CASES}
    assert 0 in EDGE_LENGTHS and {255, 256, 257} <= set(EDGE_LENGTHS) and {7, 8, 9} <= set(EDGE_LENGTHS)


@pytest.mark.parametrize("L", [0, 1, 3])
@pytest.mark.parametrize("form", ["uv", "u_only", "v_only"])
def test_the_formulas_reproduce_float64_autograd(L, form):
    """z_0 = W0x x + t_u(p): the tangent-form formulas with dt_u = sum over the row of zbar_0 give autograd's gradients of
    the table-as-leaf network to 1e-12 of the largest entry; and from dt, d c_u = W0c^T dt_u, d W0c = sum_u dt_u c_u^T,
    d b_0 = sum_u dt_u are autograd's of the network that folds its codes"""
    net = make_net(16, L, seed=L).double()
    lengths = [5, 0, 13, 1, 18]
    n, C = sum(lengths), 6
    code_of, _ = rows_from_lengths(lengths)
    pts = make_points(n, seed=L + 1).double()
    U, V = (t.double() for t in seeded_UV(n, seed=L))
    if form == "u_only":
        V = None
    if form == "v_only":
        U = torch.zeros_like(U)
    g = torch.Generator().manual_seed(L)
    W0c = (torch.randn(16, C, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    b0 = net.lins[0].bias.detach().clone().requires_grad_(True)
    codes = (torch.randn(len(lengths), C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    table = b0 + codes @ W0c.t()
    want = table_grads(net, table, None, code_of, pts, U, V, torch.float64)
    got = table_form_grads(net, table.detach(), code_of, pts, U, V)
    assert sorted(got) == sorted(want)
    for k in want:
        top = want[k].abs().max().item()
        assert got[k].shape == want[k].shape, k
        assert (got[k] - want[k]).abs().max().item() <= 1e-12 * max(top, 1.0), (k, top)
    assert (want["dt"][1] == 0).all() and want["dt"][3].abs().max() > 0
    # the chain over the fold
    table.backward(want["dt"])
    dt = got["dt"]
    for name, mine, auto in (("d c", dt @ W0c.detach(), codes.grad), ("d W0c", dt.t() @ codes.detach(), W0c.grad),
                             ("d b0", dt.sum(0), b0.grad)):
        top = auto.abs().max().item()
        assert top > 0 and (mine - auto).abs().max().item() <= 1e-12 * max(top, 1.0), name


@pytest.mark.parametrize("case", ["sorted", "shuffled", "empty_rows", "out_of_range"])
def test_cloud_order(case):
    from iso_points_amd.sdf_models import cloud_order
    U = 5
    if case == "sorted":
        idx = torch.tensor([0, 0, 1, 2, 2, 2, 3, 4, 4])
    elif case == "shuffled":
        idx = torch.tensor([3, 0, 4, 2, 0, 1, 2, 4, 2], dtype=torch.int32)
    elif case == "empty_rows":
        idx = torch.tensor([3, 3, 1, 3, 1])
    else:
        idx = torch.tensor([7, -1, 2, 100, 0, -5, 4])
    clamped = idx.long().clamp(0, U - 1)
    order, inverse, code_of, code_first = cloud_order(idx, U)
    n = idx.numel()
    assert order.dtype == torch.int64 and code_of.dtype == torch.int32 and code_first.dtype == torch.int64
    assert code_first.shape == (U + 1,) and code_first[0] == 0 and code_first[-1] == n
    assert torch.equal(code_of.long(), clamped[order]) and (code_of[1:] >= code_of[:-1]).all()
    assert torch.equal(order[inverse], torch.arange(n)) and torch.equal(inverse[order], torch.arange(n))
    assert torch.equal(code_of.long()[inverse], clamped)
    for u in range(U):
        members = torch.nonzero(clamped == u).reshape(-1)
        lo, hi = int(code_first[u]), int(code_first[u + 1])
        assert hi - lo == members.numel() and torch.equal(order[lo:hi], members)        # stable: a row keeps its order
    if case == "sorted":
        assert torch.equal(order, torch.arange(n))


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from iso_points_amd import _lib, sdf_models

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(_lib, "load", no_call)
    model = sdf_models.Siren(hidden_size=16, n_layers=1, c_dim=4)
    pts = torch.zeros(10, 3)
    c = torch.zeros(2, 4)
    idx = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(ValueError, match="not both"):
        sdf_models.siren_forward(model, pts, c=c, cloud_idx=idx, lengths=[5, 5])
    for bad in ([5, 4], [5, 5, 0], [11, -1], [10]):
        with pytest.raises(ValueError, match="lengths"):
            sdf_models.siren_forward(model, pts, c=c, lengths=bad)
    for bad_c in (torch.zeros(2, 5), torch.zeros(4), torch.zeros(2, 1, 4), None):
        with pytest.raises(ValueError, match="codes"):
            sdf_models.siren_forward(model, pts, c=bad_c, lengths=[5, 5])
    for bad_idx in (torch.zeros(9, dtype=torch.int64), torch.zeros(10)):
        with pytest.raises(ValueError, match="cloud_idx"):
            sdf_models.siren_forward(model, pts, c=c, cloud_idx=bad_idx)
    with pytest.raises(ValueError, match="latent-conditioned"):
        sdf_models.siren_forward(sdf_models.Siren(hidden_size=16, n_layers=1), pts, c=c, lengths=[5, 5])
    # the pass-through is by name, not as forward kwargs
    with pytest.raises(ValueError, match="not both"):
        sdf_models.get_normals_from_grad(model, pts, c=c, cloud_idx=idx, lengths=[5, 5])
    with pytest.raises(ValueError, match="lengths"):
        sdf_models.sdf_forward(model, pts, c=c, lengths=[1, 2])
    # the good arguments get as far as the device check
    with pytest.raises(RuntimeError, match="on the GPU"):
        sdf_models.siren_forward(model, pts, c=c, lengths=[4, 6])
