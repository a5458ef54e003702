"""The fused texture network (csrc/texture.hip: k_texture_x16<256>, k_texture_x16<512>; iso_points_amd/texture.py) against
float64: every kernel instance and every extreme of the accepted shapes, the K padding of layer 0, clouds that end inside a
tile and take more than one round of workgroups, operand ranges, several clouds, determinism, the operators built on it
and the refusals of the C ABI.

Every case first asserts iso_texture_form.  CASES is also read by tests/test_texture_cpu.py, which checks without a GPU
that it reaches every k_texture_x16 instance of the built library.  The kernel has one GEMM form (split fp16), so there is
no mode to vary, and its tiles are always drawn from the counter.

The criterion is the standing one for value kernels (test_idr_gpu.py): with s = max |rgb - rgb_float64|
over the case, s_hip <= 1.5 s_ref + 2e-7, s_ref being torch's float32 forward of the same module on the same inputs
(CPU).  Every input tensor is a slice out of a NaN-filled buffer: a read past a row or past n shows as NaN."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1500
CAP_BLOCKS = 256                      # kIdrBlocks: the most workgroups a launch runs, 64 points each

# (hidden, n_layers, c_dim, geom, n_freq); n_freq = -1: no view direction
FORMS = [
    (512, 4, 256, 6, 4),              # the reference's default
    (512, 4, 0, 6, 4),
    (256, 4, 8, 6, 4),
    (256, 1, 0, 3, -1),               # every lower extreme
    (512, 8, 256, 6, 6),              # every upper extreme
    (256, 8, 256, 6, 6),
    (512, 1, 8, 6, 0),                # the raw direction
    (256, 4, 0, 3, 4),                # point and view, no normal
    (512, 4, 8, 3, -1),
    (256, 1, 256, 6, -1),
]
# K padding of layer 0: D0 = 3 | 63, 64, 65 | 301
KPAD = [(256, 2, 0, 3, -1), (256, 2, 30, 6, 4), (256, 2, 31, 6, 4), (256, 2, 32, 6, 4), (256, 2, 256, 6, 6),
        (512, 2, 31, 6, 4), (512, 2, 32, 6, 4)]
RAGGED = [(256, 1, 8, 6, 4), (512, 1, 0, 6, 0)]
CASES = FORMS + KPAD + RAGGED


def _form(shape):
    from iso_points_amd import _lib
    code = _lib.load().iso_texture_form(*shape)
    assert code == 600 + shape[0] // 16, (shape, code)
    return code


def make_net(shape, seed=0, weight_norm=True):
    from iso_points_amd.texture import RenderingNetwork
    H, NL, C, G, Fq = shape
    torch.manual_seed(seed)
    return RenderingNetwork(dim=G + (3 if Fq >= 0 else 0), c_dim=C, hidden_size=H, n_layers=NL, weight_norm=weight_norm,
                            num_frequencies=max(Fq, 0))


def clone_net(net, dtype):
    """A CPU copy of a RenderingNetwork in `dtype` (modules under nn.utils.weight_norm do not deepcopy)."""
    from iso_points_amd.texture import RenderingNetwork
    V = net.embed_fn.out_dim if net.embed_fn is not None else 0
    m = RenderingNetwork(dim=net.dim - net.c_dim - (V - 3 if V else 0), c_dim=net.c_dim, hidden_size=net.lin0.out_features,
                         n_layers=net.num_layers - 2, weight_norm=hasattr(net.lin0, "weight_g"),
                         num_frequencies=(V - 3) // 6 if V else 0)
    m.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return m.to(dtype)


def guarded(t):
    """t as a slice out of a larger NaN-filled buffer (contiguous, same values)."""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 512,), float("nan"), dtype=t.dtype) if t.is_floating_point() else \
        torch.full((flat.numel() + 512,), 2 ** 30, dtype=t.dtype)
    buf[256:256 + flat.numel()] = flat
    return buf


def on_gpu(t, dev):
    """The guarded buffer moved to the GPU, and the view of it that holds t."""
    if t is None:
        return None
    return guarded(t).to(dev)[256:256 + t.numel()].view(t.shape)


def make_inputs(shape, n, seed, n_clouds=1):
    """points in the cube, normals unnormalised with lengths in [0.3, 3], codes randn, camera centres outside the cube"""
    H, NL, C, G, Fq = shape
    g = torch.Generator().manual_seed(1000 + seed)
    pts = torch.rand(n, 3, generator=g) * 2 - 1
    nrm = None
    if G == 6:
        d = torch.randn(n, 3, generator=g)
        nrm = d / d.norm(dim=-1, keepdim=True) * (0.3 + 2.7 * torch.rand(n, 1, generator=g))
    c = torch.randn(n, C, generator=g) if C else None
    cams = idx = None
    if Fq >= 0:
        cams = torch.randn(n_clouds, 3, generator=g)
        cams = cams / cams.norm(dim=-1, keepdim=True) * 3.0
        if n_clouds > 1:                                   # ragged: every cloud half the size of the one before, the first the rest
            sizes = [n >> (k + 1) for k in range(1, n_clouds)]
            sizes = [n - sum(sizes)] + sizes
            idx = torch.repeat_interleave(torch.arange(n_clouds), torch.tensor(sizes)).to(torch.int32)
    return pts, nrm, c, cams, idx


def torch_rgb(net, inp, dtype):
    """The module's own torch forward on the CPU in `dtype`, rows as NeuralTexture builds them."""
    from iso_points_amd.texture import texture_rows
    pts, nrm, c, cams, idx = inp
    m = clone_net(net, dtype)
    with torch.no_grad():
        x = texture_rows(m, pts.to(dtype), None if nrm is None else nrm.to(dtype), None if cams is None else cams.to(dtype), idx)
        return m(x, c=None if c is None else c.to(dtype)).rgb


def hip_rgb(net, inp, dev):
    from iso_points_amd.texture import texture_rgb
    pts, nrm, c, cams, idx = [on_gpu(t, dev) for t in inp]
    out = texture_rgb(net.to(dev), pts, nrm, c, cams, idx)
    torch.cuda.synchronize()
    return out.cpu()


def assert_margin(rgb, r32, r64, what):
    assert torch.isfinite(rgb).all(), "%s: non-finite output" % (what,)
    s_ref = (r32.double() - r64).abs().max().item()
    s_hip = (rgb.double() - r64).abs().max().item()
    print("%s: s_ref %.3g s_hip %.3g" % (what, s_ref, s_hip))
    assert s_hip <= 1.5 * s_ref + 2e-7, (what, s_ref, s_hip)
    assert rgb.min().item() >= 0.0 and rgb.max().item() <= 1.0


def check(shape, net, inp, dev, what=None):
    _form(shape)
    rgb = hip_rgb(net, inp, dev)
    assert_margin(rgb, torch_rgb(net, inp, torch.float32), torch_rgb(net, inp, torch.float64), what or (shape,))
    return rgb


@pytest.mark.parametrize("shape", FORMS)
def test_forms(dev, shape):
    check(shape, make_net(shape, seed=shape[1]), make_inputs(shape, N, seed=shape[2]), dev)


def test_weights_perturbed_after_folding(dev):
    """A weight-normed network folded into a plain one, then every weight moved by 0.01 randn."""
    from iso_points_amd.sdf_models import _effective_weight
    shape = (512, 4, 8, 6, 4)
    wn, plain = make_net(shape, seed=3), make_net(shape, seed=4, weight_norm=False)
    with torch.no_grad():
        for l in range(wn.num_layers - 1):
            a, b = getattr(wn, "lin%d" % l), getattr(plain, "lin%d" % l)
            b.weight.copy_(_effective_weight(a) + 0.01 * torch.randn_like(b.weight))
            b.bias.copy_(a.bias + 0.01 * torch.randn_like(b.bias))
    check(shape, plain, make_inputs(shape, N, seed=5), dev, "perturbed")


@pytest.mark.parametrize("shape", KPAD)
def test_k_padding_of_layer_0(dev, shape):
    H, NL, C, G, Fq = shape
    assert C + G + (3 + 6 * Fq if Fq >= 0 else 0) in (3, 63, 64, 65, 301)
    check(shape, make_net(shape, seed=C), make_inputs(shape, N, seed=C + 1), dev)


@pytest.mark.parametrize("shape", RAGGED)
def test_ragged_ends_and_rounds(dev, shape):
    """One workgroup-cap's worth of tiles plus 65 points; the same points in slices give the same bits: no point's
    arithmetic depends on its tile neighbours."""
    n = CAP_BLOCKS * 64 + 65
    net, inp = make_net(shape, seed=7), make_inputs(shape, n, seed=8)
    full = check(shape, net, inp, dev, (shape, n))
    for lo, hi in ((0, 1), (0, 63), (0, 64), (0, 65), (0, 130), (100, 230), (n - 65, n)):
        part = tuple(t if (t is None or t.shape[0] != n) else t[lo:hi].contiguous() for t in inp)
        got = hip_rgb(net, part, dev)
        assert got.shape == (hi - lo, 3) and torch.equal(got, full[lo:hi]), (shape, lo, hi)


def test_range_weights_times_50(dev):
    """tanh saturates and most ReLUs are dead or huge."""
    shape = (256, 4, 8, 6, 4)
    net = make_net(shape, seed=9, weight_norm=False)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(50.0)
    check(shape, net, make_inputs(shape, N, seed=10), dev, "weights x 50")


def test_range_codes_times_1000(dev):
    """Codes of the order of 1e3: the input row's per-point scale.  Finite, and the standing margin.  (Layer 0's
    pre-activations are of the order of 500 here; this is the case that shows how the accumulator is rounded: with the
    three partial products in one pass it missed the margin)"""
    shape = (512, 4, 256, 6, 4)
    pts, nrm, c, cams, idx = make_inputs(shape, N, seed=11)
    check(shape, make_net(shape, seed=12), (pts, nrm, c * 1.0e3, cams, idx), dev, "codes x 1e3")


@pytest.mark.parametrize("shape", [(256, 2, 0, 6, 4), (512, 2, 8, 6, 0)])
def test_point_at_its_camera_centre(dev, shape):
    pts, nrm, c, cams, idx = make_inputs(shape, 200, seed=13)
    pts[17] = cams[0]
    pts[199] = cams[0]
    rgb = check(shape, make_net(shape, seed=14), (pts, nrm, c, cams, idx), dev, (shape, "at the centre"))
    assert torch.isfinite(rgb[[17, 199]]).all()


def test_several_clouds(dev):
    """Three ragged clouds with three camera centres through cloud_idx, against torch per cloud."""
    shape = (256, 3, 8, 6, 4)
    net, inp = make_net(shape, seed=15), make_inputs(shape, N, seed=16, n_clouds=3)
    pts, nrm, c, cams, idx = inp
    sizes = torch.bincount(idx.long(), minlength=3)
    assert sizes.min() > 0 and len(set(sizes.tolist())) == 3
    rgb = check(shape, net, inp, dev, "three clouds")
    for k in range(3):                                   # per cloud: one centre, no index
        sel = idx == k
        one = (pts[sel], nrm[sel], c[sel], cams[k:k + 1], None)
        assert_margin(rgb[sel], torch_rgb(net, one, torch.float32), torch_rgb(net, one, torch.float64), "cloud %d" % k)
        assert torch.equal(hip_rgb(net, one, dev), rgb[sel])


def test_two_calls_give_identical_bits(dev):
    shape = (512, 4, 256, 6, 4)
    net, inp = make_net(shape, seed=17), make_inputs(shape, 5000, seed=18)
    _form(shape)
    assert torch.equal(hip_rgb(net, inp, dev), hip_rgb(net, inp, dev))


# ---- operators -------------------------------------------------------------------------------
def test_neural_texture_branches(dev):
    """NeuralTexture.forward: points alone | [normals, points] | with the view direction, against the module's own torch
    forward."""
    from iso_points_amd.texture import NeuralTexture
    g = torch.Generator().manual_seed(19)
    lens = [300, 500, 200]
    cams3 = torch.randn(3, 3, generator=g) * 2
    for shape, view_dependent, use_cams in (((256, 2, 0, 3, -1), False, False), ((256, 2, 8, 6, -1), False, True),
                                            ((256, 2, 8, 6, -1), True, False), ((256, 2, 8, 6, 4), True, True)):
        _form(shape)
        net = make_net(shape, seed=20)
        pts, nrm, c, _, _ = make_inputs(shape, sum(lens), seed=21)
        idx = torch.repeat_interleave(torch.arange(3), torch.tensor(lens))
        cams = cams3 if (view_dependent and use_cams) else None
        tex = NeuralTexture(net.to(dev), view_dependent=view_dependent)
        assert tex.decoder.dim == shape[2] + shape[3] + (3 + 6 * shape[4] if shape[4] >= 0 else 0)
        got = tex(on_gpu(pts, dev), on_gpu(nrm, dev), c=on_gpu(c, dev), camera_centers=cams3.to(dev) if use_cams else None,
                  lengths=lens).cpu()
        ref = (pts, nrm if shape[3] == 6 else None, c, cams, idx if cams is not None else None)
        assert_margin(got, torch_rgb(net, ref, torch.float32), torch_rgb(net, ref, torch.float64), (shape, view_dependent))


def test_unsupported_width_takes_torch_with_one_warning(dev):
    from iso_points_amd import _lib, texture as T
    shape = (128, 2, 8, 6, 4)
    assert _lib.load().iso_texture_form(*shape) == -1
    net = make_net(shape, seed=22).to(dev)
    assert T.texture_spec(net) is None
    pts, nrm, c, cams, idx = [None if t is None else t.to(dev) for t in make_inputs(shape, 300, seed=23)]
    T._TORCH_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a = T.texture_rgb(net, pts, nrm, c, cams)
        b = T.texture_rgb(net, pts, nrm, c, cams)
    assert len([w for w in rec if "no fused texture kernel" in str(w.message)]) == 1
    with torch.no_grad():
        want = net(T.texture_rows(net, pts, nrm, cams), c=c).rgb
    assert torch.equal(a, want) and torch.equal(b, want)


def test_weights_changed_in_place_change_the_result(dev):
    """No packed image survives a call: an in-place update through .data (which bumps no version counter) is seen."""
    from iso_points_amd.texture import PackedTexture, texture_rgb
    shape = (256, 2, 0, 6, 4)
    net = make_net(shape, seed=24).to(dev)
    pts, nrm, c, cams, idx = [None if t is None else t.to(dev) for t in make_inputs(shape, 300, seed=25)]
    first = texture_rgb(net, pts, nrm, c, cams)
    held = PackedTexture(net, dev)
    net.lin2.bias.data.add_(0.5)
    second = texture_rgb(net, pts, nrm, c, cams)
    assert (second - first).abs().max().item() > 1e-3
    assert torch.equal(texture_rgb(net, pts, nrm, c, cams, packed=held), first)      # the caller's image, on their word
    inp = (pts.cpu(), nrm.cpu(), None, cams.cpu(), None)
    assert_margin(second.cpu(), torch_rgb(net, inp, torch.float32), torch_rgb(net, inp, torch.float64), "updated")


def test_vertex_colors_on_a_sphere_mesh(dev):
    from iso_points_amd.ops import marching_tetrahedra, sdf_grid
    from iso_points_amd.sdf_models import Siren, SphereSDF, siren_sdf_and_grad
    from iso_points_amd.texture import NeuralTexture, texture_rgb, vertex_colors
    shape = (256, 2, 0, 6, 4)
    _form(shape)
    values, origin, spacing = sdf_grid(SphereSDF(radius=0.6).to(dev), 16)
    verts, faces = marching_tetrahedra(values, origin, spacing)
    assert verts.shape[0] > 300 and faces.shape[0] > 0
    torch.manual_seed(26)
    sdf = Siren(hidden_size=64, n_layers=2).to(dev)
    tex = NeuralTexture(make_net(shape, seed=27).to(dev))
    cam = torch.tensor([[0.0, 0.5, -3.0]], device=dev)
    got = vertex_colors(sdf, tex, verts, camera_centers=cam, points_batch_size=250)
    normals = siren_sdf_and_grad(sdf, verts, need_grad=True)[1]
    want = texture_rgb(tex.decoder, verts, normals, None, cam).clamp(0.0, 1.0)
    assert got.shape == (verts.shape[0], 3) and torch.equal(got, want)
    assert (normals.norm(dim=-1) > 0).all()


def test_raytrace_image_on_a_sphere(dev):
    from iso_points_amd.ray_tracing import RayTracing
    from iso_points_amd.sdf_models import FusedSdf, SphereSDF
    from iso_points_amd.texture import NeuralTexture, raytrace_image, texture_rgb
    shape = (256, 2, 0, 6, 4)
    _form(shape)
    sphere = SphereSDF(radius=0.5).to(dev)
    tex = NeuralTexture(make_net(shape, seed=28).to(dev))
    axis = torch.linspace(-0.3, 0.3, 32)
    yy, xx = torch.meshgrid(axis, axis, indexing="ij")
    dirs = torch.nn.functional.normalize(torch.stack([xx, yy, torch.ones_like(xx)], dim=-1).reshape(-1, 3), dim=-1).to(dev)
    cam = torch.tensor([0.0, 0.0, -3.0], device=dev)
    mask_in = torch.ones(32 * 32, dtype=torch.bool, device=dev)
    tracer = RayTracing().eval()
    rgba = raytrace_image(sphere, tex, cam, dirs, mask_in, ray_tracer=tracer)
    pts, mask, _ = tracer(FusedSdf(sphere, dev), cam.view(1, 3), mask_in, dirs.view(1, -1, 3))
    mask = mask.reshape(-1)
    assert rgba.shape == (32 * 32, 4) and 50 < int(mask.sum()) < 32 * 32 - 50
    assert torch.equal(rgba[:, 3] > 0, mask) and torch.equal(rgba[:, 3], mask.float())
    hits = pts.reshape(-1, 3)[mask].contiguous()
    x = hits.clone().requires_grad_(True)
    normals = torch.autograd.grad(sphere(x).sdf.sum(), x)[0]
    want = texture_rgb(tex.decoder, hits, normals, None, cam.view(1, 3))
    assert torch.equal(rgba[mask][:, :3], want)
    assert (rgba[~mask] == 0).all()


# ---- refusals through the C ABI --------------------------------------------------------------
def test_abi_refusals_launch_nothing(dev):
    """Status codes of iso_texture_rgb / iso_texture_pack_weights; none of these calls reaches a launch."""
    from iso_points_amd import _lib
    lib = _lib.load()
    shape = (256, 2, 8, 6, 4)
    n = 100
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    pts, nrm, codes, cams, rgb = f(n, 3), f(n, 3), f(n, 8), f(1, 3), f(n, 3)
    packed = f(lib.iso_texture_packed_floats(*shape))
    ws = torch.zeros((lib.iso_texture_workspace_bytes(n, *shape),), dtype=torch.uint8, device=dev)
    P = _lib.ptr
    OK, INVALID, UNSUPPORTED = 0, -1, -2

    def call(shape=shape, pts=pts, nrm=nrm, codes=codes, cams=cams, idx=None, n_origins=1, rgb=rgb, n=n, packed=packed, ws=ws,
             ws_bytes=None):
        return lib.iso_texture_rgb(P(pts), P(nrm), P(codes), P(cams), P(idx), n_origins, P(rgb), n, P(packed), *shape, P(ws),
                                   ws.numel() if ws_bytes is None else ws_bytes, None)
    for bad in ((128, 2, 8, 6, 4), (384, 2, 8, 6, 4), (256, 0, 8, 6, 4), (256, 9, 8, 6, 4), (256, 2, 257, 6, 4),
                (256, 2, -1, 6, 4), (256, 2, 8, 4, 4), (256, 2, 8, 6, 7), (256, 2, 8, 6, -2)):
        assert lib.iso_texture_form(*bad) == -1
        assert call(shape=bad) == UNSUPPORTED, bad
        assert lib.iso_texture_pack_weights(P(pts), P(packed), *bad, None) == UNSUPPORTED, bad
    assert b"iso_texture" in lib.iso_last_error()
    for kw in (dict(pts=None), dict(nrm=None), dict(codes=None), dict(cams=None), dict(rgb=None), dict(packed=None),
               dict(ws=None, ws_bytes=64), dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0), dict(n_origins=0), dict(n=-1)):
        assert call(**kw) == INVALID, kw
    # a pointer where none is allowed
    assert call(shape=(256, 2, 8, 3, 4)) == INVALID and call(shape=(256, 2, 0, 6, 4)) == INVALID
    assert call(shape=(256, 2, 8, 6, -1)) == INVALID
    assert lib.iso_texture_pack_weights(None, P(packed), *shape, None) == INVALID
    assert lib.iso_texture_pack_weights(P(pts), None, *shape, None) == INVALID
    # n == 0: success without a launch, whatever the pointers
    assert call(n=0) == OK
    assert lib.iso_texture_rgb(None, None, None, None, None, 0, None, 0, None, *shape, None, 0, None) == OK
    torch.cuda.synchronize()
    assert float(rgb.abs().max()) == 0.0                                   # nothing was written
