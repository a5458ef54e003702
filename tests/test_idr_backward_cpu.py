"""The mathematics of the IDR SDF's backward (csrc/idrgrad.hip implements it), proved on the CPU: the tangent
form restated in float64 torch without autograd (tests/idr_backward_oracle.py::tangent_form_grads) against torch's double
backward of sum(U f) + sum(V . grad_x f), to 1e-10 relative per tensor; and the host-only entry points of the C ABI."""
import pytest
import torch

from idr_backward_oracle import (err, make_net, make_points, seeded_UV, shape_of, tangent_form_grads, torch_grads)

H = 16
CASES = [(nl, skip, nf) for nf in (0, 2) for nl, skips in ((2, (None, 1)), (4, (None, 1, 2))) for skip in skips]
N = 40


def _case(nl, skip, nf, seed=0):
    net = make_net(H, nl, skip, nf, seed=10 * nl + nf + seed).double()
    pts = make_points(N, seed=nl + nf)
    U, V = seeded_UV(N, nl)
    return net, pts.double(), U.double(), V.double()


def _assert_same(got, want, what, tol=1e-10):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].shape == want[k].shape, (what, k)
        assert err(got[k], want[k]) <= tol, (what, k, err(got[k], want[k]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_skip%s_F%d" % c)
def test_tangent_form_is_torchs_double_backward(case):
    nl, skip, nf = case
    net, pts, U, V = _case(*case)
    want = torch_grads(net, pts, U, V, torch.float64)
    _assert_same(tangent_form_grads(net, pts, U, V), want, case)
    # what the geometric initialisation would have hidden: the encoding columns of W_0 and of the skip layer, and dx
    D0 = 3 + 6 * nf
    assert want["points"].abs().max() > 0
    if nf > 0:
        assert want["W0"][:, 3:].abs().max() > 0
        if skip is not None:
            assert want["W%d" % skip][:, H - D0 + 3:].abs().max() > 0
    if skip is not None:
        assert want["W%d" % (skip - 1)].shape[0] == H - D0 and want["W%d" % skip][:, H - D0:].abs().max() > 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_skip%s_F%d" % c)
def test_value_only_and_gradient_only(case):
    net, pts, U, V = _case(*case, seed=3)
    _assert_same(tangent_form_grads(net, pts, U, None), torch_grads(net, pts, U, None, torch.float64), (case, "V None"))
    zero = torch.zeros_like(U)
    want = torch_grads(net, pts, zero, V, torch.float64)
    _assert_same(tangent_form_grads(net, pts, zero, V), want, (case, "U = 0"))
    # the second-order term is really there
    for k in want:
        assert want[k].abs().max() > 0, k


def test_shape_of_reads_the_oracle_module():
    assert shape_of(make_net(H, 4, 2, 2, seed=1)) == (H, 4, 2, 2) and shape_of(make_net(H, 2, None, 0, seed=1)) == (H, 2, -1, 0)


# ---- host-only entry points ----------------------------------------------------------------------------------------------
ACCEPTED = [(128, 2, -1, 0), (128, 3, 1, 4), (256, 4, 2, 6), (256, 4, 3, 10), (512, 2, -1, 6), (512, 8, 4, 6), (128, 12, 6, 6),
            (512, 12, 11, 10)]
REFUSED = [(64, 4, 2, 6), (1024, 4, 2, 6), (384, 4, 2, 6), (0, 4, 2, 6), (256, 1, -1, 6), (256, 13, 4, 6), (256, 4, 4, 6),
           (256, 4, 0, 6), (256, 4, 2, 11), (256, 4, 2, -1)]


def test_form_accepts_and_refuses():
    from iso_points_amd import _lib
    lib = _lib.load()
    for H_, nl, skip, nf in ACCEPTED:
        assert lib.iso_idrgrad_form(H_, nl, skip, nf) == 900 + H_ // 16, (H_, nl, skip, nf)
        assert lib.iso_idr_step_form(H_, nl, skip, nf, 0) > 0
    for H_, nl, skip, nf in REFUSED:
        assert lib.iso_idrgrad_form(H_, nl, skip, nf) == 0, (H_, nl, skip, nf)
        assert lib.iso_idr_step_form(H_, nl, skip, nf, 0) == -1      # the forward's own table refuses the same shapes


def test_workspace_bytes_and_chunks():
    from iso_points_amd import _lib
    lib = _lib.load()
    wsp, chunk = lib.iso_idrgrad_workspace_points(), lib.iso_idrgrad_chunk_points()
    assert wsp > 0 and chunk > 0 and wsp % chunk == 0
    for shape in REFUSED:
        assert lib.iso_idrgrad_workspace_bytes(1000, *shape) == 0, shape
    for shape in ACCEPTED:
        b = [lib.iso_idrgrad_workspace_bytes(n, *shape) for n in (0, 1, chunk, chunk + 1, wsp - 1, wsp, wsp + 1, 10 * wsp)]
        assert b[0] == b[1] > 0 and all(x < y for x, y in zip(b[1:5], b[2:6])), shape
        assert b[5] == b[6] == b[7], shape
        assert all(x % 4 == 0 for x in b)
    # the header's formula, at the reference's default network
    H_, nl, skip, nf = 512, 8, 4, 6
    raw = lib.iso_idr_raw_floats(H_, nl, skip, nf)
    want = 4 * (512 + 2 * wsp * 64 + 2 * nl * 2 * wsp * H_ + 2 * wsp + (wsp // chunk) * raw)
    assert lib.iso_idrgrad_workspace_bytes(wsp, H_, nl, skip, nf) == want == 776598784
