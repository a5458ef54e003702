"""The texture backward without a GPU: the iso_texgrad_* entries of the C ABI (header, ctypes table, library, size helpers,
iso_texgrad_form at every limit), the guard that the GPU cases reach every k_texgrad_* kernel of the built library, and the
oracle itself against the reference's own gradients (tests/golden/texture_grad_*.npz, written by
tests/golden/make_golden_texture_grad.py)."""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_texture_backward_gpu import BACKWARD_CASES
from texture_backward_oracle import fence_filter, rows_of

GOLDEN = ("wn_c8_f4.npz", "c0_f0.npz", "points_only.npz")
ENTRIES = ["iso_texgrad_backward", "iso_texgrad_chunk_points", "iso_texgrad_form", "iso_texgrad_pack_weights",
           "iso_texgrad_packed_floats", "iso_texgrad_workspace_bytes", "iso_texgrad_workspace_points"]


def _lib():
    from iso_points_amd import _lib
    return _lib.load()


def test_header_ctypes_table_and_library_agree_on_the_texgrad_entries():
    import ctypes
    from iso_points_amd import _lib
    from test_abi import declared_symbols
    names = [s for s in declared_symbols() if s.startswith("iso_texgrad_")]
    assert sorted(names) == ENTRIES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["iso_texgrad_backward"][1]) == 22              # packed_fw and packed_bw
    assert len(_lib.SIGNATURES["iso_texgrad_pack_weights"][1]) == len(_lib.SIGNATURES["iso_texture_pack_weights"][1])


SHAPES = [(256, 1, 0, 3, -1), (512, 4, 256, 6, 4), (256, 8, 31, 6, 4), (512, 2, 8, 3, 0), (512, 8, 256, 6, 6)]


@pytest.mark.parametrize("shape", SHAPES)
def test_size_helpers_need_no_gpu(shape):
    lib = _lib()
    H, NL, C, G, Fq = shape
    D0 = C + G + (3 + 6 * Fq if Fq >= 0 else 0)
    K0 = (D0 + 63) // 64 * 64
    raw = lib.iso_texture_raw_floats(*shape)
    chunk, WS_POINTS = lib.iso_texgrad_chunk_points(), lib.iso_texgrad_workspace_points()
    assert chunk >= 64 and WS_POINTS >= chunk and WS_POINTS % chunk == 0
    # header, head rows and bias, W_0^T in f32 (K0 rows), split-fp16 images of W_l^T (two halves of two parts = one float
    # per weight)
    assert lib.iso_texgrad_packed_floats(*shape) == 64 + 3 * H + 4 + K0 * H + (NL - 1) * H * H
    for n in (0, 1, 63, chunk, chunk + 1, 1500, WS_POINTS, WS_POINTS + 1, 262144):
        mw = min(max(n, 1), WS_POINTS)
        want = 4 * (mw * (K0 + 2 * NL * H + 4) + (mw + chunk - 1) // chunk * raw) + 64      # + the tile counter
        assert lib.iso_texgrad_workspace_bytes(n, *shape) == want, n
    assert lib.iso_texgrad_packed_floats(128, NL, C, G, Fq) == 0 and lib.iso_texgrad_workspace_bytes(100, 128, NL, C, G, Fq) == 0


def test_form_on_both_sides_of_every_limit():
    lib = _lib()
    form = lib.iso_texgrad_form
    assert form(256, 4, 8, 6, 4) == 716 and form(512, 4, 8, 6, 4) == 732
    for H in (0, 64, 128, 255, 257, 384, 511, 513, 1024):
        assert form(H, 4, 8, 6, 4) == -1, H
    assert [form(256, NL, 8, 6, 4) for NL in (-1, 0, 1, 8, 9)] == [-1, -1, 716, 716, -1]
    assert [form(512, 4, C, 6, 4) for C in (-1, 0, 256, 257)] == [-1, 732, 732, -1]
    assert [form(256, 4, 8, G, 4) for G in (0, 2, 3, 4, 5, 6, 7, 9)] == [-1, -1, 716, -1, -1, 716, -1, -1]
    assert [form(512, 4, 8, 6, Fq) for Fq in (-2, -1, 0, 6, 7)] == [-1, 732, 732, 732, -1]
    # the same shapes as the forward, everywhere
    for shape in [(H, NL, C, G, Fq) for H in (128, 256, 512) for NL in (0, 1, 8, 9) for C in (0, 256, 257) for G in (3, 5, 6)
                  for Fq in (-2, -1, 6, 7)]:
        assert (form(*shape) >= 0) == (lib.iso_texture_form(*shape) >= 0), shape


def test_gpu_cases_reach_every_texgrad_kernel_of_the_library():
    """iso_texgrad_form's code 700 + hidden / 16 names the instances k_texgrad_fwd_x16<hidden> (recompute) and
    k_texgrad_rev_x16<hidden> (reverse sweep, launched with two layers or more); the GPU cases reach exactly the instances
    the code object holds.  The other kernels take the width as an argument.  The code object must hold exactly these
    kernels: a new one without a case fails here, on the CPU."""
    from test_abi import _code_object_kernels
    plain, inst = set(), set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_texgrad_\w*)", name)
        if m:
            kernel, rest = m.group(2)[:int(m.group(1))], m.group(2)[int(m.group(1)):]
            t = re.match(r"ILi(\d+)EE", rest)
            (inst.add((kernel, int(t.group(1)))) if t else plain.add(kernel))
    # the reduce: csrc/grad_sums.hip, tests/test_grad_sums_cpu.py
    assert plain == {"k_texgrad_stats", "k_texgrad_pack", "k_texgrad_head", "k_texgrad_dx", "k_texgrad_tn",
                     "k_texgrad_bias", "k_texgrad_head_partial"}, sorted(plain)
    assert inst == {("k_texgrad_fwd_x16", 256), ("k_texgrad_fwd_x16", 512), ("k_texgrad_rev_x16", 256),
                    ("k_texgrad_rev_x16", 512)}, sorted(inst)
    lib = _lib()
    assert all(lib.iso_texgrad_form(*s) == 700 + s[0] // 16 for s in BACKWARD_CASES)
    reached = {16 * (lib.iso_texgrad_form(*s) - 700) for s in BACKWARD_CASES}
    assert reached == {h for k, h in inst if k == "k_texgrad_fwd_x16"} == {h for k, h in inst if k == "k_texgrad_rev_x16"}
    # the reverse instance runs only with two layers or more: both widths have such a case
    assert {s[0] for s in BACKWARD_CASES if s[1] >= 2} == reached
    assert any(s[1] >= 2 for s in BACKWARD_CASES) and any(s[1] == 1 for s in BACKWARD_CASES)
    for i, ends in enumerate(((256, 512), (1, 8), (0, 256), (3, 6), (-1, 0, 6))):
        assert set(ends) <= {c[i] for c in BACKWARD_CASES}, (i, ends)


@pytest.mark.parametrize("name", GOLDEN)
def test_oracle_reproduces_the_reference_gradients(name):
    """texture.RenderingNetwork under rows_of (the oracle's row assembly) and torch autograd in float64 gives the gradients
    the reference's network gave under its own NeuralTexture.forward."""
    from iso_points_amd.texture import RenderingNetwork
    z = np.load(os.path.join(ROOT, "tests", "golden", "texture_" + name))
    zg = np.load(os.path.join(ROOT, "tests", "golden", "texture_grad_" + name))
    net = RenderingNetwork(dim=int(z["dim"]), c_dim=int(z["c_dim"]), hidden_size=int(z["hidden"]), n_layers=int(z["n_layers"]),
                           weight_norm=bool(z["weight_norm"]), num_frequencies=int(z["num_frequencies"]))
    net.load_state_dict(OrderedDict((k[3:], torch.from_numpy(z[k])) for k in z.files if k.startswith("sd/")), strict=True)
    net = net.double()
    with_view, points_only = bool(z["with_view"]), int(z["dim"]) == 3
    p = torch.from_numpy(z["points"]).double().requires_grad_(True)
    nrm = None if points_only else torch.from_numpy(z["normals"]).double().requires_grad_(True)
    c = torch.from_numpy(z["codes"]).double().requires_grad_(True) if int(z["c_dim"]) else None
    cams = torch.from_numpy(z["cams"]).double() if with_view else None
    x = rows_of(net, p, nrm, cams, torch.from_numpy(z["cloud"]) if with_view else None)
    (net(x, c=c).rgb * torch.from_numpy(zg["G"])).sum().backward()
    names = sorted(k[5:] for k in zg.files if k.startswith("grad/"))
    assert names == sorted(k for k, _ in net.named_parameters())
    for k, v in net.named_parameters():
        want = torch.from_numpy(zg["grad/" + k])
        assert (v.grad - want).abs().max().item() <= 1e-12,k
    for t, key in ((p, "grad_points"), (nrm, "grad_normals"), (c, "grad_codes")):
        if t is not None:
            want = torch.from_numpy(zg[key])
            assert want.shape == t.shape and (t.grad - want).abs().max().item() <= 1e-12,key
    assert p.grad.abs().max().item() > 0


@pytest.mark.parametrize("shape", [(256, 1, 0, 3, -1), (512, 4, 256, 6, 4), (256, 8, 256, 6, 6), (512, 8, 256, 6, 6), (256, 2, 31, 6, 4)])
def test_fence_filter_keeps_nearly_everything(shape):
    from test_texture_gpu import make_inputs, make_net
    net = make_net(shape, seed=1)
    inp, kept = fence_filter(net, make_inputs(shape, 1500, seed=2))
    print(shape, kept)
    assert 0.97 <= kept <= 1.0
    assert all(t is None or t is inp[3] or t.shape[0] == round(kept * 1500) for t in inp)
