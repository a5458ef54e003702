"""Every path of the splat backward kernels (iso_points_amd/csrc/splat_backward.hip) against the float64 reference of
splat_backward_oracle.py, on images past one 64 x 64 super block.

xy gradient, per point and component:  |got - ref64| <= (n_terms + 8) * 2^-24 * abs_sum + unc_sum  (derived in the
oracle's docstring; exactly +0.0 where the point has no term); z gradient, per point:  |got - exact| <= n_p * q / 2 +
(2^-24 + 2^-50) * |exact|  with q the fixed-point step the comment above k_z_scatter promises.  Every call runs twice
and must repeat bit for bit.  That each case reaches the path it is there for, and that at most 2 % of its points see
an uncertain pixel, is asserted on the CPU (test_splat_backward_cpu.py).

Left out: the second iteration of the light kernel's `i0` loop (it needs more than 8 M points in one cloud: the grid
is capped at 8192 workgroups of 1024 points), the image-side limit of 2048 and the refusal paths.

Observed on an MI355X (worst |got - ref| / bound of the xy gradient; points with an uncertain pixel; census of
splat_backward_oracle.path_census: heavy / light-and-zero points, dense-row / bit-scan blocks, points with a second word
round, with more than one block-row round, with a read at cx = NB2x - 1 in the last block row of the last cloud):

  case       image     worst   uncertain   heavy   light0  dense   scan    word>1  rows>1  last-word
  a          72x72     0.290   0 / 600     395     0       0       2099    0       36      0
  b          72x72     0.022   1 / 600     394     0       4201    0       0       30      0
  c_sparse   130x67    0.107   0 / 600     386     0       0       7200    0       316     0
  c_dense    130x67    0.009   0 / 600     395     0       0       9313    0       335     0
  d1_sparse  72x328    0.019   0 / 400     258     0       0       45526   114     258     49
  d2_dense   72x328    0.001   0 / 400     273     0       52798   0       71      273     24
  e          200x136   0.243   0 / 500     91      229     0       1499    0       87      0
  f_dense    136x200   0.020   0 / 500     313     0       14423   0       0       223     0
  f_ring     136x200   0.159   1 / 500     325     0       1539    5626    0       289     0
  g_disc     64x64     0.113   0 / 64      64      0       0       484     0       0       16
  g_rect     64x64     0.126   0 / 64      64      0       0       823     0       21      25
  h          72x72     0.381   2 / 140001  135822  0       -       -       0       0       1554   (two heavy strides)
  j: a, d1_sparse misaligned: bit for bit the aligned result; b misaligned 0.021
  full path (a, d1_sparse, c_sparse x K = 5, 8): xy 0.08 - 0.19, no uncertain point

z gradient: worst |got - exact| / bound 0.95 - 1.00 in every set but `steps` (0 - 0.57) -- the bound is the float32
rounding of the exact sum plus the fixed-point step, and the result is that rounding.  (On a 72-row image a disc
of 1.6 spans 16 blocks: case d takes 4.0 -- 37 blocks -- for one cloud to reach the second word round.)
"""
import numpy as np
import pytest
import torch

import splat_backward_oracle as O
from splat_util import random_splats

pytestmark = pytest.mark.gpu

EXTRA = 5          # rows behind the last cloud: they belong to no cloud and keep the zeros of the result


def _backward(dev, c, go=None, misaligned=False, idx=None, gz=None):
    """_C._backward on a case, twice; -> (P + EXTRA, 3) on the host"""
    from iso_points_amd.rasterizer import _C
    go = (c["go"] if go is None else go).to(dev)
    if misaligned:                     # a contiguous view one float into a larger buffer
        buf = torch.zeros(go.numel() + 8, device=dev)
        view = buf[1:1 + go.numel()].view(go.shape)
        view.copy_(go)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        go = view
    pad = lambda t, v: torch.cat([t, torch.full((EXTRA,) + tuple(t.shape[1:]), v, dtype=t.dtype)]).to(dev)
    pts, radii = pad(c["points"], 0.25), pad(c["radii"], 0.05)             # (the extra rows would see gradient pixels)
    vis = pad(c["visible"], 1) if c["visible"] is not None else None
    kw = dict(visible=vis, rs=c["rs"].to(dev) if c["rs"] is not None else None, rect_mode=int(c["rect"]),
              radii_s=c["radii_s"], idx=idx, grad_zbuf=gz)
    first, num = c["first"].to(dev), c["num"].to(dev)
    got = _C._backward(pts, radii, go, first, num, **kw).cpu()
    again = _C._backward(pts, radii, go, first, num, **kw).cpu()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs differ"
    return got


def _check_xy(name, got, ref):
    """the per-point bound; -> worst |got - ref| / bound"""
    P = ref.n_terms.size
    xy = got[:P, :2].numpy().astype(np.float64)
    err, bound = np.abs(xy - ref.grad), O.occ_bound(ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s: worst |got - ref| / bound = %.4f over %d points with terms; uncertain points %d of %d" % (
        name, worst, (ref.n_terms > 0).sum(), (ref.n_unc > 0).sum(), P))
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d components past the bound (first point %d), worst %.3g x" % (
        name, bad.sum(), np.nonzero(bad.any(axis=1))[0][0], worst)
    none = (ref.n_terms == 0) & (ref.n_unc == 0)
    assert none.any() or name.startswith("g_")
    bits = got[:P, :2].contiguous().view(torch.int32).numpy()
    assert not bits[none].any(), "%s: a point without terms is not exactly +0.0" % name
    assert not got[P:].view(torch.int32).any(), "%s: rows outside every cloud were written" % name
    return worst


@pytest.mark.parametrize("name", O.CASES)
def test_xy_gradient_within_the_derived_bound(dev, name):
    """cases a - h of the table in splat_backward_oracle.case"""
    c, ref = O.case(name), O.case_ref(name)
    got = _backward(dev, c)
    _check_xy(name, got, ref)
    assert not got[:, 2].any()                                  # no z gradient was asked for
    if name.startswith("g_"):
        assert not ref.unc_sum.any()


@pytest.mark.parametrize("name", ["a", "f_dense"])
def test_zero_gradient_image(dev, name):
    """case i: heavy count 0, every gradient exactly +0.0 (disc and rectangle support)"""
    c = O.case(name)
    got = _backward(dev, c, go=torch.zeros_like(c["go"]))
    assert not got.view(torch.int32).any()


@pytest.mark.parametrize("name", ["a", "d1_sparse", "b"])
def test_misaligned_gradient_image(dev, name):
    """case j: the base pointer of grad_occ is 4 bytes past a 16-byte boundary, every 16-byte path is refused.  The
    terms and the lanes that add them are the same on the bit-scan path (a, d1_sparse): bit for bit the aligned
    result there; the dense case (b) changes lanes and is held to the bound."""
    c, ref = O.case(name), O.case_ref(name)
    got = _backward(dev, c, misaligned=True)
    _check_xy(name + " misaligned", got, ref)
    if name != "b":
        assert O.case_census(name)["dense_blocks"] == 0
        assert torch.equal(got.view(torch.int32), _backward(dev, c).view(torch.int32))


# ------------------------------------------------------------------------------------------------ z gradient
def _z_sets(shape, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(shape, generator=g)
    sparse = base.clone()
    sparse[torch.rand(shape, generator=g) < 0.6] = 0.0
    wide = torch.sign(base) * 10.0 ** (torch.rand(shape, generator=g) * 60 - 30)
    tiny = base / base.abs().max() * 1e-38
    # odd multiples of the step q that a largest value of 1.0 gives: every term and every sum is an exact multiple of q,
    # so the fixed-point sum is exact and a step that is one bit coarser is off by q in every term (the float rounding
    # of a sum of random values hides that: 2^-24 |sum| is far above n_p q / 2)
    q = 2.0 ** -(61 - int(np.ceil(np.log2(shape[1] * shape[2]))) - 1)
    steps = torch.sign(base) * (2 * torch.randint(0, 1 << 15, shape, generator=g) + 1).float() * q
    steps.view(-1)[0] = 1.0
    return {"normal": base, "zeros60": sparse, "all_zero": torch.zeros(shape), "wide": wide, "denormal": tiny,
            "steps": steps}


def _check_z(what, got_z, idx, gz, P, pixels_per_view, poisoned=()):
    exact, n_p = O.zbuf_backward_exact(idx, gz, P)
    q = O.z_quantum(gz, pixels_per_view)
    z = got_z.numpy().astype(np.float64)
    nan = np.isnan(exact)
    assert sorted(np.nonzero(nan)[0].tolist()) == sorted(poisoned), what
    assert np.array_equal(np.isnan(z), nan), "%s: NaN on other points than the poisoned ones" % what
    ok = ~nan
    err, bound = np.abs(z[ok] - exact[ok]), O.z_bound(exact[ok], n_p[ok], q)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s: worst |got - exact| / bound = %.4f, q = 2^%d, most terms %d" % (
        what, worst, int(np.log2(q)) if q else 0, n_p.max()))
    assert (err <= bound).all(), "%s: %d points past the bound, worst %.3g x" % (what, (err > bound).sum(), worst)
    assert not got_z[torch.from_numpy(n_p == 0)].view(torch.int32).any(), what      # exactly +0.0 without a term
    return worst


def _z_case(H, W, N, P, seed):
    g = torch.Generator().manual_seed(seed)
    pts, radii, _ = O._rand_points(g, P, H, W)
    first, num = O._split(P, N)
    return dict(points=pts, radii=radii, visible=None, go=torch.zeros(N, H, W), first=first, num=num,
                rs=torch.full((N,), 0.1), rect=False, radii_s=10.0)


@pytest.mark.parametrize("H,W", [(72, 72), (130, 67)])
@pytest.mark.parametrize("K", [1, 4, 5, 8])
def test_z_gradient_exactly_rounded(dev, H, W, K):
    """K % 4 == 0: the 16-byte path, else the scalar one; lists with a random -1 suffix, points listed in thousands of
    pixels; magnitudes from the denormal range to 1e30; a NaN and an Inf poison exactly their points."""
    N, P = 2, 900
    c = _z_case(H, W, N, P, 7 * K + H)
    idx = O.synthetic_lists(N, H, W, K, P, 100 + K + W)
    sets = _z_sets((N, H, W, K), K + H)
    # one NaN and one Inf, each on a point of its own, in slots that count (not behind a -1, which no list has in slot 0)
    poison = sets["normal"].clone()
    filled = torch.nonzero(idx[..., 0].reshape(-1) >= 0).reshape(-1)
    pa, pb = P // 2 + 1, P // 2 + 2
    flat_i, flat_g = idx.reshape(-1, K).clone(), poison.reshape(-1, K)
    flat_i[filled[3], 0], flat_i[filled[-3], 0] = pa, pb
    flat_g[filled[3], 0], flat_g[filled[-3], 0] = float("nan"), float("-inf")
    idx_p = flat_i.reshape(idx.shape)
    for what, ii, gz, bad in [(k, idx, v, ()) for k, v in sets.items()] + [("nan_inf", idx_p, poison, (pa, pb))]:
        got = _backward(dev, c, idx=ii.to(dev), gz=gz.to(dev))
        assert not got[:, :2].any()
        _check_z("z %dx%d K=%d %s" % (H, W, K, what), got[:P, 2], ii, gz, P, H * W, bad)
        if what == "all_zero":
            assert not got.view(torch.int32).any()
        if what == "wide":
            assert got[:P, 2].abs().max() > 1e29


@pytest.mark.parametrize("K", [4, 8])
def test_z_gradient_misaligned_lists_take_the_scalar_path(dev, K):
    """idx and grad_zbuf one element into a larger buffer: the 16-byte path is refused; bit for bit the aligned result"""
    H, W, N, P = 72, 72, 2, 900
    c = _z_case(H, W, N, P, K)
    idx = O.synthetic_lists(N, H, W, K, P, 200 + K)
    gz = _z_sets((N, H, W, K), 300 + K)["zeros60"]
    want = _backward(dev, c, idx=idx.to(dev), gz=gz.to(dev))
    bi = torch.full((idx.numel() + 8,), -1, dtype=torch.int32, device=dev)
    bg = torch.zeros(gz.numel() + 8, device=dev)
    vi, vg = bi[1:1 + idx.numel()].view(idx.shape), bg[1:1 + gz.numel()].view(gz.shape)
    vi.copy_(idx)
    vg.copy_(gz)
    assert vi.data_ptr() % 16 == 4 and vg.data_ptr() % 16 == 4 and vi.is_contiguous() and vg.is_contiguous()
    got = _backward(dev, c, idx=vi, gz=vg)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    _check_z("z misaligned K=%d" % K, got[:P, 2], idx, gz, P, H * W)


def test_z_pieces_equal_the_whole(dev):
    """The entry points of the multi-rank path on three row bands of a 72 x 328 x 8 case: absmax / scatter into two
    accumulators / integer add / finish, and the band calls over two views -- the z column of the single call bit for
    bit, and iso_splat_mark_visible's marks."""
    from iso_points_amd import _lib
    p = _lib.ptr
    H, W, K, N, P = 72, 328, 8, 2, 3000
    c = _z_case(H, W, N, P, 5)
    idx = O.synthetic_lists(N, H, W, K, P, 6).to(dev)
    gz = _z_sets((N, H, W, K), 8)["zeros60"].to(dev)
    want = _backward(dev, c, idx=idx, gz=gz)[:P, 2]
    _check_z("z pieces, whole", want, idx.cpu(), gz.cpu(), P, H * W)
    bands = [(0, 20), (20, 48), (48, 72)]
    # pieces: every band of every view is a contiguous piece
    zs = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.call("iso_splat_z_absmax", p(gz), gz.numel(), p(zs), _lib.stream())
    acc = [torch.zeros(P, dtype=torch.int64, device=dev) for _ in range(2)]
    for t, (v, (y0, y1)) in enumerate([(v, b) for v in range(N) for b in bands]):
        _lib.call("iso_splat_z_scatter", p(idx[v, y0:y1]), p(gz[v, y0:y1]), (y1 - y0) * W, K, H * W, p(zs), p(acc[t % 2]),
                  _lib.stream())
    assert acc[0].any() and acc[1].any()
    grad = torch.zeros(P, 3, device=dev)
    _lib.call("iso_splat_z_finish", p(acc[0] + acc[1]), p(zs), 0, P, p(grad), _lib.stream())
    assert torch.equal(grad[:, 2].cpu().view(torch.int32), want.view(torch.int32)) and not grad[:, :2].any()
    # bands of both views in one call each
    vis = torch.zeros(P, dtype=torch.uint8, device=dev)
    zb = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in bands]
    for z, (y0, y1) in zip(zb, bands):
        _lib.call("iso_splat_band_marks", p(idx[0, y0:y1]), p(gz[0, y0:y1]), N, H * W, (y1 - y0) * W, K, p(vis), p(z),
                  _lib.stream())
    zmax = torch.stack(zb).max(dim=0).values.contiguous()                  # the MAX reduction over the ranks
    assert zmax[0].item() == zs[0].item()
    acc2 = torch.zeros(P, dtype=torch.int64, device=dev)
    for y0, y1 in bands:
        _lib.call("iso_splat_band_z_scatter", p(idx[0, y0:y1]), p(gz[0, y0:y1]), N, H * W, (y1 - y0) * W, K, p(zmax),
                  p(acc2), _lib.stream())
    assert torch.equal(acc2, acc[0] + acc[1])
    grad2 = torch.zeros(P, 3, device=dev)
    _lib.call("iso_splat_z_finish", p(acc2), p(zmax), 0, P, p(grad2), _lib.stream())
    assert torch.equal(grad2[:, 2].cpu().view(torch.int32), want.view(torch.int32))
    vis_ref = torch.zeros(P, dtype=torch.uint8, device=dev)
    _lib.call("iso_splat_mark_visible", p(idx), N * H * W, K, p(vis_ref), _lib.stream())
    assert torch.equal(vis, vis_ref)
    assert np.array_equal(vis.cpu().numpy() != 0, O.visible_and_radius(idx.cpu(), c["radii"], c["first"], c["num"], 10.0)[0])


# ------------------------------------------------------------------------------------------------ the full path
@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("name", ["a", "d1_sparse", "c_sparse"])
def test_full_path_through_the_autograd_op(dev, name, K):
    """EllipticalRasterizer.apply on the image and gradient of a case: idx from the GPU forward (pinned bit for bit
    elsewhere), the visible set and median radius restated on the host, xy and z held to the bounds above."""
    from iso_points_amd.rasterizer import EllipticalRasterizer, _visible_and_radius
    go = O.case(name)["go"]
    N, H, W = go.shape
    sc = random_splats(600, N=N, seed=K + N + H)
    m = min(H, W)
    ndc = (sc["ndc"] * torch.tensor([W / m, H / m, 1.0])).contiguous()
    P = ndc.shape[0]
    gz = _z_sets((N, H, W, K), K + W)["zeros60"]
    first, num = sc["first"].to(dev), sc["num"].to(dev)
    dv = lambda k: sc[k].to(dev)

    def run():
        pts = ndc.to(dev).requires_grad_(True)
        oi, oz, _, oo = EllipticalRasterizer.apply(pts, dv("ellipse"), dv("cutoff"), dv("radii"), first, num, 0.05, (H, W),
                                                   K, 0, 0, 10.0)
        ((oo * go.to(dev)).sum() + (oz * gz.to(dev)).sum()).backward()
        return oi, pts.grad.cpu()

    oi, got = run()
    assert torch.equal(run()[1].view(torch.int32), got.view(torch.int32))
    idx = oi.cpu()
    vis, rs = O.visible_and_radius(idx, sc["radii"], sc["first"], sc["num"], 10.0)
    vis_d, rs_d = _visible_and_radius(oi, dv("radii"), first, num, 10.0)
    assert np.array_equal(vis_d.cpu().numpy() != 0, vis) and 50 < vis.sum() < P
    assert np.array_equal(rs_d.cpu().numpy(), rs) and (rs > 0).all()
    ref = O.occ_backward64(ndc, sc["radii"], go, sc["first"], sc["num"], rs=torch.from_numpy(rs),
                           visible=torch.from_numpy(vis.astype(np.uint8)))
    assert (ref.n_unc > 0).sum() <= 0.02 * P and (ref.n_terms > 0).sum() > 50
    what = "full path %s K=%d" % (name, K)
    _check_xy(what, torch.cat([got, torch.zeros(EXTRA, 3)]), ref)
    _check_z(what, got[:, 2], idx, gz, P, H * W)
