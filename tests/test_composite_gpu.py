"""Compositing on the GPU, every kernel form, forward and backward, against the float64 restatement in
tests/composite_oracle.py (checked on the CPU by tests/test_composite_cpu.py).  Every comparison with float64 applies
the derived bounds of composite_oracle.bounds element by element, no element excluded, and asserts error / bound <= 1.

Largest error / bound measured on an MI355X (this file, all cases; the float32 restatement on the CPU gives 0.302,
0.245, 0.123, 0.067):
    image 0.247, grad_q 0.209, grad_features 0.126, grad_scaler 0.067

Which kernel a call runs cannot be read back through the C ABI, so the tests restate the dispatch rule of
iso_splat_composite (_register_form) and assert its inputs: the pointers' alignment, K and C."""
import numpy as np
import pytest
import torch

import composite_oracle as CO

pytestmark = pytest.mark.gpu

EPS = CO.EPS
WORST = {"image": 0.0, "grad_q": 0.0, "grad_features": 0.0, "grad_scaler": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ncompositing, largest error / bound over this run: " + ", ".join("%s %.3f" % kv for kv in WORST.items()))


_REF = {}


def _reference(key, s, norm):
    """float64 backward (with the forward and the companions inside), computed once per (set, norm) and never changed."""
    if (key, norm) not in _REF:
        _REF[(key, norm)] = CO.backward(s["idx"], s["q"], s["occ"], s["scaler"], s["feat"], norm, EPS, s["grad_img"])
    return _REF[(key, norm)]


def _shape(n_pix):
    return (1, 37, 29) if n_pix == CO.N_FORM else (1, n_pix, 1)


def _offset_view(t):
    """The same values in a contiguous view one element into a larger allocation: 4 bytes off a 16-byte boundary."""
    buf = torch.empty((t.numel() + 8,), dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (t.numel() == 0 or v.data_ptr() % 16 == 4)
    return v


def _to_dev(s, dev):
    n_pix, K = s["idx"].shape
    hw = _shape(n_pix)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    t["idx"], t["q"], t["occ"] = t["idx"].view(hw + (K,)), t["q"].view(hw + (K,)), t["occ"].view(hw)
    t["grad_img"] = t["grad_img"].view(hw + (-1,))
    return t


def _register_form(K, C, *tensors):
    """The dispatch rule of iso_splat_composite (include/isopoints.h): the register kernels take K = 4 or 8 with at
    most 3 channels when idx, qvalue (and frag_scaler_out) are 16-byte aligned; the generic kernel everything else."""
    return K in (4, 8) and C <= 3 and all(x.data_ptr() % 16 == 0 for x in tensors)


def _composite(t, norm, need=("q", "occ", "scaler", "feat"), idx=None, q=None, backward=True):
    """composite() and its backward on device tensors -> image, {name: grad or None}."""
    from iso_points_amd.rasterizer import PointFragments, composite
    # (detach() makes a new leaf on the same memory: an offset view stays an offset view)
    leaf = {"q": (t["q"] if q is None else q).detach(), "occ": t["occ"].detach(), "scaler": t["scaler"].detach(),
            "feat": t["feat"].detach()}
    for k in need:
        leaf[k].requires_grad_(True)
    img = composite(PointFragments(t["idx"] if idx is None else idx, None, leaf["q"], None, leaf["occ"]), leaf["scaler"],
                    leaf["feat"], norm_weighted=norm, eps=EPS)
    if not backward:
        return img, None
    img.backward(t["grad_img"])
    return img.detach(), {k: leaf[k].grad for k in leaf}


def _direct(t, norm, frag_scaler=None):
    """iso_splat_composite called through the C ABI, as composite() did before it learned to chunk."""
    from iso_points_amd import _lib
    K, C = t["idx"].shape[-1], t["feat"].shape[1]
    out = torch.empty(t["idx"].shape[:-1] + (C + 1,), dtype=torch.float32, device=t["idx"].device)
    p = _lib.ptr
    _lib.call("iso_splat_composite", p(t["idx"]), p(t["q"]), p(t["occ"]), p(t["scaler"]), p(t["feat"]),
              t["occ"].numel(), K, C, int(norm), EPS, p(frag_scaler), p(out), _lib.stream())
    return out


def _check(name, got, ref, bound):
    r = CO.ratio(got, ref, bound)
    print("%s error / bound = %.3f" % (name, r))
    WORST[name] = max(WORST[name], r)
    assert r <= 1.0, (name, r)


def _check_all(img, grads, bw, K, C, chunks=1, names=("image", "grad_q", "grad_features", "grad_scaler")):
    b = CO.bounds(bw, K, C, chunks)
    fw = bw["forward"]
    n_pix = fw["image"].shape[0]
    if "image" in names:
        _check("image", img.reshape(n_pix, C + 1)[:, :C], fw["image"][:, :C], b["image"])
        assert np.array_equal(img.reshape(n_pix, C + 1)[:, C].cpu().numpy().astype(np.float64), fw["image"][:, C])
    if "grad_q" in names:
        _check("grad_q", grads["q"].reshape(n_pix, K), bw["grad_q"], b["grad_q"])
    if "grad_features" in names:
        _check("grad_features", grads["feat"], bw["grad_features"], b["grad_features"])
    if "grad_scaler" in names:
        _check("grad_scaler", grads["scaler"], bw["grad_scaler"], b["grad_scaler"])
    if grads is not None and grads.get("occ") is not None:
        assert np.array_equal(grads["occ"].reshape(-1).cpu().numpy().astype(np.float64), bw["grad_occ"])


# ------------------------------------------------------------------------------------- (a) every stand-alone form
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("C", CO.FORM_C)
@pytest.mark.parametrize("K", CO.FORM_K)
def test_every_form_forward_and_backward_vs_float64(dev, K, C, norm):
    s = CO.form_set(K, C)
    t = _to_dev(s, dev)
    # fresh allocations are aligned, so the rule selects the register kernels exactly at K in {4, 8}, C <= 3
    assert t["idx"].data_ptr() % 16 == 0 and t["q"].data_ptr() % 16 == 0
    assert _register_form(K, C, t["idx"], t["q"]) == (K in (4, 8) and C <= 3)
    img, grads = _composite(t, norm)
    assert img.shape == (1, 37, 29, C + 1)
    _check_all(img, grads, _reference(("form", K, C), s, norm), K, C)
    # at most 8 channels: composite() is the one launch it always was
    assert torch.equal(img, _direct(t, norm))


# ------------------------------------------------------------------------------------- (b) register form = generic form
@pytest.mark.parametrize("C", [0, 1, 3])
@pytest.mark.parametrize("K", [4, 8])
def test_register_form_is_the_generic_form_bit_for_bit(dev, K, C):
    s = CO.form_set(K, C)
    t = _to_dev(s, dev)
    for norm in (True, False):
        assert _register_form(K, C, t["idx"], t["q"])
        a = _direct(t, norm)
        assert torch.equal(a, _direct(t, norm)), "the register form does not reproduce itself"
        for which in ("idx", "q"):
            u = dict(t)
            u[which] = _offset_view(t[which])
            assert not _register_form(K, C, u["idx"], u["q"])
            b = _direct(u, norm)
            assert torch.equal(a, b), "misaligned %s, norm_weighted=%s: %d values differ" % (which, norm, (a != b).sum().item())
        img, _ = _composite(t, norm, idx=_offset_view(t["idx"]), backward=False)
        assert torch.equal(a, img.detach())


# ------------------------------------------------------------------------------------- (c) the clamp, the cancellation
@pytest.mark.parametrize("K", [1, 8])
def test_clamped_and_empty_pixels_and_the_k1_cancellation(dev, K):
    s = CO.clamp_set(K)
    bw = _reference(("clamp", K), s, True)
    fw = bw["forward"]
    nonempty = (s["idx"] >= 0).any(1)
    assert 0.3 <= (~fw["through"])[nonempty].mean() <= 0.7 and (~nonempty).mean() >= 0.10
    if K == 1:                               # float64: dL/dw is exactly 0 where the one fragment passes through
        assert np.abs(bw["grad_q"][fw["through"]]).max() < 1e-12 * bw["Gq"].max()
    img, grads = _composite(_to_dev(s, dev), True)
    _check_all(img, grads, bw, K, 3)
    empty = torch.from_numpy(~nonempty).to(dev).view(1, 37, 29)
    assert (img[empty][:, :3] == 0).all() and (grads["q"][empty] == 0).all()


# ------------------------------------------------------------------------------------- (d) dead-slot garbage
@pytest.mark.parametrize("K", [4, 6, 8])
def test_dead_slots_are_never_read(dev, K):
    s_nan, s_neg = CO.garbage_set(K), CO.garbage_set(K, dead_q=-1.0)
    assert np.isnan(s_nan["q"]).any() and not np.isnan(s_neg["q"]).any()
    for norm in (True, False):
        bw = _reference(("garbage", K), s_nan, norm)
        img_a, ga = _composite(_to_dev(s_nan, dev), norm)
        img_b, gb = _composite(_to_dev(s_neg, dev), norm)
        for x in (img_a, img_b) + tuple(ga.values()) + tuple(gb.values()):
            assert torch.isfinite(x).all()
        assert torch.equal(img_a, img_b) and torch.equal(ga["q"], gb["q"]) and torch.equal(ga["occ"], gb["occ"])
        _check_all(img_a, ga, bw, K, 3)
        _check_all(img_b, gb, bw, K, 3)


# ------------------------------------------------------------------------------------- (e) contention
def test_twenty_thousand_pixels_scatter_to_one_point(dev):
    s = CO.contention_set()
    bw = _reference("contention", s, True)
    assert bw["n_p"][0] >= 20000
    img, grads = _composite(_to_dev(s, dev), True)
    _check_all(img, grads, bw, 8, 3)


# ------------------------------------------------------------------------------------- (f) the stride loop's second trip
@pytest.mark.parametrize("norm", [True, False])
def test_more_pixels_than_one_grid_of_threads(dev, norm):
    """iso_stream_grid caps the generic forward kernel and the backward kernel at 4096 blocks of 256: pixels past
    1,048,576 are a thread's second trip."""
    s = CO.stride_set()
    assert s["idx"].shape[0] > 4096 * 256
    img, grads = _composite(_to_dev(s, dev), norm)
    _check_all(img, grads, _reference("stride", s, norm), 1, 1)


# ------------------------------------------------------------------------------------- (g) needs_input_grad subsets
def test_every_subset_of_requested_gradients(dev):
    s = CO.subset_set()
    t = _to_dev(s, dev)
    bw = _reference("subsets", s, True)
    img, full = _composite(t, True)
    _check_all(img, full, bw, 6, 3)
    for need in (("feat",), ("scaler",), ("q",), ("occ",), ("feat", "scaler")):
        _, g = _composite(t, True, need=need)
        for k in ("q", "occ", "scaler", "feat"):
            assert (g[k] is not None) == (k in need), (need, k)
        names = [{"feat": "grad_features", "scaler": "grad_scaler", "q": "grad_q"}[k] for k in need if k != "occ"]
        _check_all(img, g, bw, 6, 3, names=names)
        if "q" in need:
            assert torch.equal(g["q"], full["q"])
        if "occ" in need:
            assert torch.equal(g["occ"], full["occ"]) and torch.equal(g["occ"], t["grad_img"][..., 3])


# ------------------------------------------------------------------------------------- (h) frag_scaler_out
@pytest.mark.parametrize("K", [8, 4, 6])
def test_frag_scaler_out_is_the_gather(dev, K):
    from iso_points_amd.rasterizer import gather_with_neg_idx
    s = CO.form_set(K, 3)
    t = _to_dev(s, dev)
    fs = torch.full(t["idx"].shape, float("nan"), dtype=torch.float32, device=dev)
    assert _register_form(K, 3, t["idx"], t["q"], fs) == (K in (4, 8))
    img = _direct(t, True, frag_scaler=fs)
    want = gather_with_neg_idx(t["scaler"], t["idx"])
    assert torch.equal(fs, want) and torch.equal(want.cpu(), torch.from_numpy(
        np.where(s["idx"] >= 0, s["scaler"][np.maximum(s["idx"], 0)], np.float32(0))).view(want.shape))
    assert torch.equal(img, _direct(t, True))
    if K in (4, 8):                          # a misaligned frag_scaler_out alone sends the call to the generic kernel
        fs2 = _offset_view(torch.full(t["idx"].shape, float("nan"), dtype=torch.float32, device=dev))
        assert torch.equal(_direct(t, True, frag_scaler=fs2), img) and torch.equal(fs2, want)


# ------------------------------------------------------------------------------------- (i) the fused epilogue
_SCENE = {}


def _scene():
    if not _SCENE:
        from splat_util import sphere_scene
        _SCENE["sc"] = sphere_scene(1500, n_views=1, S=32)
    return _SCENE["sc"]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("C", [1, 8])
@pytest.mark.parametrize("K", [5, 8, 40])
def test_fused_epilogue_at_other_channel_counts(dev, K, C, norm):
    from iso_points_amd.rasterizer import _C, PointFragments, composite
    sc = _scene()
    P = sc["ndc"].shape[0]
    feat = torch.from_numpy(np.random.default_rng(C).standard_normal((P, C)).astype(np.float32)).to(dev)
    scal = sc["scaler"].to(dev)
    args = [sc[k].to(dev) for k in ("ndc", "ellipse", "cutoff", "radii", "first", "num")]
    idx, zb, qv, occ, img = _C.splat_points(*args, 0.05, 32, K, composite_with=(scal, feat, norm, 1e-4))
    assert (idx >= 0).float().mean() > 0.05 and occ.sum() > 50
    want = composite(PointFragments(idx, zb, qv, None, occ), scal, feat, norm_weighted=norm, eps=1e-4)
    assert torch.equal(img, want), "%d values differ" % (img != want).sum().item()
    if K == 8 and C == 8:
        fw = CO.forward(idx, qv, occ, scal, feat, norm, EPS)
        _check("image", img.reshape(-1, C + 1)[:, :C], fw["image"][:, :C], CO.image_bound(fw, K))
        assert torch.equal(img[..., C], occ)


# ------------------------------------------------------------------------------------- (j) gather_with_neg_idx
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1024, 1025])
def test_gather_with_neg_idx_aligned_and_offset(dev, n):
    from iso_points_amd.rasterizer import gather_with_neg_idx
    rng = np.random.default_rng(n)
    values = torch.from_numpy(rng.standard_normal(50).astype(np.float32)).to(dev)
    idx = torch.from_numpy(rng.integers(-20, 50, size=n).astype(np.int32)).to(dev)
    if n >= 3:
        idx[n - 1] = -1
        idx[0] = 49
    want = torch.where(idx >= 0, values[idx.long().clamp(min=0)], torch.zeros((), device=dev))
    assert torch.equal(gather_with_neg_idx(values, idx), want)
    off = _offset_view(idx)                  # contiguous, int32, 4 bytes off: the kernel refuses it, the function must not
    got = gather_with_neg_idx(values, off)
    assert got.shape == want.shape and torch.equal(got, want)


# ------------------------------------------------------------------------------------- (k) int64 idx, wide features
@pytest.mark.parametrize("K", [6, 8])
def test_int64_idx_is_converted(dev, K):
    """The reference's renderer composites fragments.idx.long(); the kernels read int32."""
    s = CO.form_set(K, 3)
    t = _to_dev(s, dev)
    img, g = _composite(t, True)
    img64, g64 = _composite(t, True, idx=t["idx"].long())
    assert torch.equal(img, img64) and torch.equal(g["q"], g64["q"]) and torch.equal(g["occ"], g64["occ"])
    bw = _reference(("form", K, 3), s, True)
    _check_all(img64, g64, bw, K, 3)


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("K", [6, 8])
def test_sixteen_channels_in_chunks_vs_float64(dev, K, norm):
    """SurfaceSplatting.forward carries 16-channel features; the kernels take 8: composite() runs two chunks."""
    s = CO.wide_set(K)
    t = _to_dev(s, dev)
    img, grads = _composite(t, norm)
    assert img.shape == (1, 37, 29, 17)
    _check_all(img, grads, _reference(("wide", K), s, norm), K, 16, chunks=2)
    # each half is the single launch on its channels
    for c0 in (0, 8):
        u = dict(t)
        u["feat"] = t["feat"][:, c0:c0 + 8].contiguous()
        assert torch.equal(img[..., c0:c0 + 8], _direct(u, norm)[..., :8])
    # the chunked backward with some outputs not requested
    bw = _reference(("wide", K), s, norm)
    for need in (("scaler",), ("feat",), ("q", "occ")):
        _, g = _composite(t, norm, need=need)
        for k in ("q", "occ", "scaler", "feat"):
            assert (g[k] is not None) == (k in need), (need, k)
        names = [{"feat": "grad_features", "scaler": "grad_scaler", "q": "grad_q"}[k] for k in need if k != "occ"]
        _check_all(img, g, bw, K, 16, chunks=2, names=names)
        if "q" in need:
            assert torch.equal(g["q"], grads["q"]) and torch.equal(g["occ"], t["grad_img"][..., 16])
