"""The texture network without a GPU: RenderingNetwork and the row assembly of NeuralTexture against the reference's own
outputs (tests/golden/texture_*.npz, written by tests/golden/make_golden_texture.py), texture_spec on both sides of what
the fused kernel covers, the new entries of the C ABI (header, ctypes table, size helpers, iso_texture_form at every limit)
and the guard that the cases of tests/test_texture_gpu.py reach every k_texture_x16 instance of the built library."""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_texture_gpu import CASES

GOLDEN = ("texture_wn_c8_f4.npz", "texture_c0_f0.npz", "texture_points_only.npz")


def _lib():
    from iso_points_amd import _lib
    return _lib.load()


def _golden(name):
    from iso_points_amd.texture import RenderingNetwork
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    net = RenderingNetwork(dim=int(z["dim"]), c_dim=int(z["c_dim"]), hidden_size=int(z["hidden"]), n_layers=int(z["n_layers"]),
                           weight_norm=bool(z["weight_norm"]), num_frequencies=int(z["num_frequencies"]))
    sd = OrderedDict((k[3:], torch.from_numpy(z[k])) for k in z.files if k.startswith("sd/"))
    net.load_state_dict(sd, strict=True)
    t = {k: torch.from_numpy(z[k]) for k in ("points", "normals", "codes", "cams", "cloud", "rows", "rgb", "rgb64")}
    return z, net, t


@pytest.mark.parametrize("name", GOLDEN)
def test_reference_state_dict_loads_strictly_and_reproduces_the_output(name):
    from iso_points_amd.texture import texture_rows
    z, net, t = _golden(name)
    assert sorted(net.state_dict().keys()) == sorted(k[3:] for k in z.files if k.startswith("sd/"))
    with_view, points_only = bool(z["with_view"]), int(z["dim"]) == 3
    assert net.dim == t["rows"].shape[1] + int(z["c_dim"]) and net.c_dim == int(z["c_dim"]) and net.num_layers == int(z["n_layers"]) + 2
    assert (net.embed_fn is not None) == (int(z["num_frequencies"]) > 0)
    for dtype, want, tol in ((torch.float64, t["rgb64"], 1e-12), (torch.float32, t["rgb"], 1e-6)):
        m = net.to(dtype)
        with torch.no_grad():
            x = texture_rows(m, t["points"].to(dtype), None if points_only else t["normals"].to(dtype),
                             t["cams"].to(dtype) if with_view else None, t["cloud"] if with_view else None)
            c = t["codes"].to(dtype) if int(z["c_dim"]) else None
            got = m(x, c=c).rgb
        assert got.dtype == dtype and got.shape == want.shape
        assert (got.double() - want.double()).abs().max().item() <= tol, (name, dtype)
        if dtype == torch.float32:
            # the rows the reference's decoder was given, the point at its camera centre (row 5) included
            assert x.shape == t["rows"].shape and (x - t["rows"]).abs().max().item() <= 1e-6
            G0 = 3 if points_only else 6
            assert torch.equal(x[:, :G0], t["rows"][:, :G0])
            if with_view:
                assert torch.equal(t["points"][5], t["cams"][0]) and torch.isfinite(x[5]).all()
                assert torch.equal(x[5, 6:9], torch.zeros(3))
    assert got.min().item() >= 0.0 and got.max().item() <= 1.0


def test_neural_texture_refuses_cpu_tensors():
    from iso_points_amd.texture import NeuralTexture, raytrace_image, texture_rgb, vertex_colors
    _, net, t = _golden("texture_wn_c8_f4.npz")
    with pytest.raises(RuntimeError):
        texture_rgb(net, t["points"], t["normals"], t["codes"], t["cams"], t["cloud"])
    with pytest.raises(RuntimeError):
        NeuralTexture(net)(t["points"], t["normals"], c=t["codes"], camera_centers=t["cams"], cloud_idx=t["cloud"])
    with pytest.raises(RuntimeError):
        vertex_colors(None, NeuralTexture(net), t["points"])
    with pytest.raises(RuntimeError):
        raytrace_image(None, NeuralTexture(net), t["cams"][0], t["normals"], torch.ones(t["normals"].shape[0], dtype=torch.bool))


def _net(**kw):
    from iso_points_amd.texture import RenderingNetwork
    args = dict(dim=9, c_dim=8, hidden_size=256, n_layers=2, weight_norm=True, num_frequencies=4)
    args.update(kw)
    return RenderingNetwork(**args)


def test_texture_spec():
    from iso_points_amd.texture import texture_spec
    import torch.nn as nn
    for wn in (True, False):
        net = _net(weight_norm=wn)
        Ws, bs, H, NL, C, G, Fq = texture_spec(net)
        assert (H, NL, C, G, Fq) == (256, 2, 8, 6, 4) and len(Ws) == len(bs) == 3
        assert [tuple(W.shape) for W in Ws] == [(256, 8 + 6 + 27), (256, 256), (3, 256)]
        assert torch.equal(Ws[1], net.lin1.weight) or wn
    # the new-style parametrization of weight-norm
    net = _net(weight_norm=False)
    for l in range(3):
        nn.utils.parametrizations.weight_norm(getattr(net, "lin%d" % l))
    spec = texture_spec(net)
    assert spec is not None and spec[2:] == (256, 2, 8, 6, 4)
    assert torch.allclose(spec[0][0], net.lin0.weight)
    # folded weights of the old style are g v / |v|
    net = _net()
    v, g = net.lin0.weight_v, net.lin0.weight_g
    assert torch.allclose(texture_spec(net)[0][0], g * v / v.norm(dim=1, keepdim=True), atol=0, rtol=1e-6)
    assert texture_spec(_net(hidden_size=512, n_layers=8, c_dim=256, num_frequencies=6))[2:] == (512, 8, 256, 6, 6)
    assert texture_spec(_net(n_layers=1, c_dim=0, dim=3, num_frequencies=0))[2:] == (256, 1, 0, 3, -1)
    assert texture_spec(_net(dim=6, num_frequencies=0))[2:] == (256, 2, 8, 6, -1)
    assert texture_spec(_net(dim=9, num_frequencies=0))[2:] == (256, 2, 8, 6, 0)
    assert texture_spec(_net(dim=6, num_frequencies=2))[2:] == (256, 2, 8, 3, 2)
    # outside the kernel
    assert texture_spec(_net(out_dims=OrderedDict(rgb=3, latent=4))) is None
    assert texture_spec(_net(out_dims=OrderedDict(latent=3))) is None
    assert texture_spec(_net(hidden_size=128)) is None
    assert texture_spec(_net(c_dim=257)) is None and texture_spec(_net(c_dim=256)) is not None
    assert texture_spec(_net(num_frequencies=7)) is None and texture_spec(_net(num_frequencies=6)) is not None
    assert texture_spec(_net(n_layers=9)) is None and texture_spec(_net(n_layers=8)) is not None
    assert texture_spec(_net(dim=12)) is None
    assert texture_spec(nn.Linear(3, 3)) is None


def test_header_ctypes_table_and_library_agree_on_the_texture_entries():
    import ctypes
    from iso_points_amd import _lib
    from test_abi import declared_symbols
    names = [s for s in declared_symbols() if s.startswith("iso_texture_")]
    assert sorted(names) == ["iso_texture_form", "iso_texture_pack_weights", "iso_texture_packed_floats",
                             "iso_texture_raw_floats", "iso_texture_rgb", "iso_texture_workspace_bytes"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["iso_texture_rgb"][1]) == 17


SHAPES = [(256, 1, 0, 3, -1), (512, 4, 256, 6, 4), (256, 8, 31, 6, 4), (512, 2, 8, 3, 0), (512, 8, 256, 6, 6)]


@pytest.mark.parametrize("shape", SHAPES)
def test_size_helpers_need_no_gpu(shape):
    lib = _lib()
    H, NL, C, G, Fq = shape
    D0 = C + G + (3 + 6 * Fq if Fq >= 0 else 0)
    assert lib.iso_texture_raw_floats(*shape) == (H * D0 + H) + (NL - 1) * (H * H + H) + (3 * H + 3)
    K0 = (D0 + 63) // 64 * 64
    assert K0 <= 320
    # header, K-order biases, head rows and bias, split-fp16 images (two halves of two parts = one float per weight)
    assert lib.iso_texture_packed_floats(*shape) == 64 + NL * H + 3 * H + 4 + K0 * H + (NL - 1) * H * H
    assert lib.iso_texture_workspace_bytes(1000, *shape) >= 4
    assert lib.iso_texture_raw_floats(128, NL, C, G, Fq) == 0 and lib.iso_texture_packed_floats(128, NL, C, G, Fq) == 0


def test_form_on_both_sides_of_every_limit():
    lib = _lib()
    form = lib.iso_texture_form
    ok = (256, 4, 8, 6, 4)
    assert form(*ok) == 616 and form(512, 4, 8, 6, 4) == 632
    for H in (0, 64, 128, 255, 257, 384, 511, 513, 1024):
        assert form(H, 4, 8, 6, 4) == -1, H
    assert [form(256, NL, 8, 6, 4) for NL in (-1, 0, 1, 8, 9)] == [-1, -1, 616, 616, -1]
    assert [form(512, 4, C, 6, 4) for C in (-1, 0, 256, 257)] == [-1, 632, 632, -1]
    assert [form(256, 4, 8, G, 4) for G in (0, 2, 3, 4, 5, 6, 7, 9)] == [-1, -1, 616, -1, -1, 616, -1, -1]
    assert [form(512, 4, 8, 6, Fq) for Fq in (-2, -1, 0, 6, 7)] == [-1, 632, 632, 632, -1]
    assert form(512, 8, 256, 6, 6) == 632 and form(256, 1, 0, 3, -1) == 616                 # D0 = 301 and D0 = 3


def test_gpu_cases_reach_every_texture_kernel_of_the_library():
    """CASES (every shape tests/test_texture_gpu.py launches through its form tests) taken through iso_texture_form reach
    exactly the k_texture_x16 instances the code object holds: a new instance without a case fails here, on the CPU."""
    from test_abi import _code_object_kernels
    in_library = set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_texture_x16)ILi(\d+)EE", name)
        if m and len(m.group(2)) == int(m.group(1)):
            in_library.add(int(m.group(3)))
    lib = _lib()
    reached = set()
    for shape in CASES:
        code = lib.iso_texture_form(*shape)
        assert code == 600 + shape[0] // 16, shape
        reached.add(16 * (code - 600))
    assert in_library == {256, 512}, sorted(in_library)
    assert reached == in_library
    # every argument extreme appears in a case
    for i, ends in enumerate(((256, 512), (1, 8), (0, 256), (3, 6), (-1, 0, 6))):
        assert set(ends) <= {c[i] for c in CASES}, (i, ends)
