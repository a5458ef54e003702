"""The float64 reference of the splat backward pass (splat_backward_oracle.py) against the C oracle and against
itself, and the conditions on the inputs of the GPU cases (test_splat_backward_gpu.py): few uncertain pixels, and
every case reaches the kernel path it is there for.  No GPU."""
import numpy as np
import pytest
import torch

import splat_backward_oracle as O
from oracle import splat_oracle as SO
from splat_util import sphere_scene


def _square_scene(S, P, seed, radius=(0.01, 0.12)):
    g = torch.Generator().manual_seed(seed)
    pts, radii, visible = O._rand_points(g, P, S, S)
    radii = radii / 0.12 * radius[1]
    go = O._grad(g, 2, S, S, 0.3)
    first, num = O._split(P, 2)
    return pts, radii.contiguous(), visible, go, first, num


def _assert_within(got, ref, what):
    err, bound = np.abs(np.asarray(got, np.float64) - ref.grad), O.occ_bound(ref)
    bad = err > bound
    assert not bad.any(), "%s: %d components past the bound, worst %.3g x" % (
        what, bad.sum(), (err[bad] / np.maximum(bound[bad], 1e-300)).max())
    assert (ref.n_terms > 0).sum() > 20 and np.abs(ref.grad).sum() > 0, what


@pytest.mark.parametrize("S,seed", [(48, 1), (37, 2), (16, 3)])
def test_oracle64_against_the_c_oracle_disc(S, seed):
    pts, radii, visible, go, first, num = _square_scene(S, 300, seed)
    rs = torch.tensor([0.35, 0.2])
    c32 = SO.occ_backward(pts, radii, go, first, num, 10.0, rs=rs, visible=visible, mode=2)
    ref = O.occ_backward64(pts, radii, go, first, num, rs=rs, visible=visible)
    _assert_within(c32.numpy(), ref, "disc S=%d" % S)
    skipped = (visible == 0) | (pts[:, 2] < 0) | (pts[:, :2].abs() > 1).any(dim=1)
    assert skipped.any() and not ref.n_terms[skipped.numpy()].any() and not c32[skipped].any()


@pytest.mark.parametrize("S,seed,radii_s", [(48, 4, 6.0), (33, 5, 10.0)])
def test_oracle64_against_the_c_oracle_rectangle(S, seed, radii_s):
    pts, radii, visible, go, first, num = _square_scene(S, 300, seed)
    c32 = SO.occ_backward(pts, radii, go, first, num, radii_s, mode=1)
    ref = O.occ_backward64(pts, radii, go, first, num, rect=True, radii_s=radii_s)
    _assert_within(c32.numpy(), ref, "rectangle S=%d" % S)


@pytest.mark.skipif(not SO.ref_available(), reason="oracle/_ref not built")
def test_oracle64_rectangle_against_the_compiled_reference():
    """The reference's CPU rule rejects with `&&`, the kernel's with `||`: they select the same pixels where the
    support covers the image in both axes (here rx, ry >= 0.25 times 10 > 2, the widest |dx|).  The ellipse-box rule
    (a positive gradient outside contributes nothing) still cuts."""
    pts, radii, visible, go, first, num = _square_scene(40, 200, 6)
    radii = (0.25 + radii).contiguous()
    c32 = SO.occ_backward(pts, radii, go, first, num, 10.0, mode=0, use_ref=True)
    ref = O.occ_backward64(pts, radii, go, first, num, rect=True, radii_s=10.0)
    _assert_within(c32.numpy(), ref, "compiled reference")
    live = ref.n_terms > 0
    assert (ref.n_terms[live] < (go != 0).sum(dim=(1, 2)).max().item()).all()        # the box rule dropped pixels


@pytest.mark.parametrize("H,W,rect", [(20, 33, False), (33, 20, True), (17, 40, False)])
def test_windowed_oracle_equals_the_full_image_evaluation(H, W, rect):
    g = torch.Generator().manual_seed(H * 100 + W)
    pts, radii, visible = O._rand_points(g, 60, H, W)
    go = O._grad(g, 2, H, W, 0.5)
    first, num = O._split(60, 2)
    kw = dict(rs=None if rect else torch.tensor([0.3, 0.55]), visible=visible, rect=rect, radii_s=4.0)
    a = O.occ_backward64(pts, radii, go, first, num, **kw)
    b = O.occ_backward64_full(pts, radii, go, first, num, **kw)
    for k in ("n_terms", "n_unc", "n_tie", "n_zero_dist"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.n_terms > 0).sum() > 10 and (a.n_terms == 0).sum() > 5
    # the same terms, summed in another (pairwise) order
    tol = 64 * 2.0 ** -53 * np.maximum(b.abs_sum, b.unc_sum)
    for k in ("grad", "abs_sum", "unc_sum"):
        assert (np.abs(getattr(a, k) - getattr(b, k)) <= tol).all(), k


@pytest.mark.parametrize("K", [1, 5, 8])
def test_exact_z_sum_against_the_c_oracle(K):
    P, S = 500, 40
    idx = O.synthetic_lists(2, S, S, K, P, K)
    gz = torch.randn(2, S, S, K, generator=torch.Generator().manual_seed(10 + K))
    gz[gz.abs() < 0.4] = 0.0
    exact, n_p = O.zbuf_backward_exact(idx, gz, P)
    mass, _ = O.zbuf_backward_exact(idx, gz.abs(), P)
    c32 = SO.zbuf_backward(idx, gz, P).numpy().astype(np.float64)
    assert n_p.max() > 100                                                  # the points that head many lists
    assert (np.abs(c32 - exact) <= n_p * 2.0 ** -24 * mass).all()          # a sequential float32 sum of n_p terms
    # a list ends at the first idx < 0 and zeros are skipped: count them by hand for one point
    valid = (torch.cumprod((idx >= 0).long(), dim=-1) != 0) & (gz != 0)
    p = int(idx[..., 0].max())
    assert n_p[p] == int(((idx == p) & valid).sum()) and n_p.sum() == int(valid.sum())


def test_exact_z_sum_poison_and_cancellation():
    idx = torch.tensor([[[[0, 1, -1, 2]], [[0, 1, 2, -1]], [[3, -1, -1, -1]]]], dtype=torch.int32)      # (1,3,1,4)
    gz = torch.tensor([[[[1e30, 1.0, 5.0, 7.0]], [[-1e30, 0.0, float("inf"), 9.0]], [[float("nan"), 1.0, 1.0, 1.0]]]])
    exact, n_p = O.zbuf_backward_exact(idx, gz, 5)
    assert exact[0] == 0.0 and exact[1] == 1.0 and np.isnan(exact[2]) and np.isnan(exact[3]) and exact[4] == 0.0
    assert n_p.tolist() == [2, 1, 1, 1, 0]


def test_visible_and_radius_against_the_oracle_driver():
    S, K = 32, 5
    sc = sphere_scene(1500, n_views=2, S=S, seed=12)
    idx, zb, _, _ = SO.splat_forward(sc["ndc"], sc["ellipse"], sc["cutoff"], sc["radii"], sc["first"], sc["num"], 0.05, S, K)
    _, vis_ref, rs_ref = SO.splat_backward(sc["ndc"], sc["radii"], idx, sc["first"], sc["num"], torch.zeros(2, S, S),
                                           torch.zeros_like(zb), 10.0)
    vis, rs = O.visible_and_radius(idx, sc["radii"], sc["first"], sc["num"], 10.0)
    assert np.array_equal(vis, vis_ref.numpy()) and 0 < vis.sum() < vis.size
    assert np.array_equal(rs, rs_ref.numpy()) and (rs > 0).all()
    # a pixel whose first slot is empty marks nothing, whatever stands behind it
    idx2 = idx.clone()
    idx2[..., 0] = -1
    assert not O.visible_and_radius(idx2, sc["radii"], sc["first"], sc["num"], 10.0)[0].any()


# ------------------------------------------------------------------------------- conditions on the GPU cases
@pytest.mark.parametrize("name", O.CASES)
def test_uncertain_share_of_the_gpu_cases(name):
    """At most 2 % of a case's points see a pixel whose membership float32 may decide differently: the cap that keeps
    the unc_sum part of the bound from hiding anything.  A condition on the inputs: a seed that breaks it is changed."""
    ref = O.case_ref(name)
    share = (ref.n_unc > 0).sum() / ref.n_unc.size
    print("case %s: uncertain points %d of %d (%.3f %%), points with terms %d" % (
        name, (ref.n_unc > 0).sum(), ref.n_unc.size, 100 * share, (ref.n_terms > 0).sum()))
    assert share <= 0.02
    assert (ref.n_terms > 0).sum() >= min(40, ref.n_terms.size // 2)
    if name.startswith("g_"):
        # exactly representable throughout: nothing is uncertain, though pixels sit exactly on the thresholds
        assert not ref.n_unc.any() and not ref.unc_sum.any()
        assert ref.n_tie.sum() > 50 and ref.n_zero_dist.sum() == 64


# case -> census columns that must be non-zero (what the case is there for)
REACHES = {
    "a": ("heavy", "scan_blocks"),
    "b": ("heavy", "dense_blocks", "clip_left", "clip_right", "clip_top", "clip_bottom"),
    "c_sparse": ("heavy", "scan_blocks"),
    "c_dense": ("heavy", "scan_blocks"),
    "d1_sparse": ("heavy", "scan_blocks", "word_rounds_gt1", "last_word_reads"),
    "d2_dense": ("heavy", "dense_blocks", "word_rounds_gt1", "last_word_reads"),
    "e": ("heavy", "light_zero", "row_rounds_gt1", "scan_blocks"),
    "f_dense": ("heavy", "dense_blocks", "row_rounds_gt1"),
    "f_ring": ("heavy", "dense_blocks", "scan_blocks", "row_rounds_gt1"),
    "g_disc": ("heavy", "scan_blocks"),
    "g_rect": ("heavy", "scan_blocks"),
    "h": ("heavy", "skipped"),
}


@pytest.mark.parametrize("name", O.CASES)
def test_gpu_cases_reach_their_paths(name):
    c = O.case_census(name)
    print("case %s: %s" % (name, c))
    for k in REACHES[name]:
        assert c[k] > 0, (name, k, c)
    if name in ("a", "b"):
        assert (c["nb2x"], c["nb2y"]) == (2, 2)                       # 2 x 2 super blocks, the outer ones partial
    if name.startswith("c_"):
        assert c["dense_blocks"] == 0                                 # W % 4 != 0: the row path is refused
        cs = O.case(name)
        assert (cs["go"][0].numel() * 4) % 16 != 0                    # cloud 1's image is not 16-byte aligned
    if name.startswith("d"):
        assert c["nb2x"] == 6
    if name == "e":
        assert c["light_zero"] > c["heavy"]                           # most points are light and zero
    if name.startswith("f_"):
        cs = O.case(name)
        full = (cs["radii"].min(dim=1).values * cs["radii_s"] > 2 * 200 / 136)
        assert full.any() or c["row_rounds_gt1"] > 100                # supports covering the image
    if name == "h":
        assert c["heavy"] > 131072 and c["heavy_strides"] == 2
        assert c["heavy"] % 64 != 0


@pytest.mark.parametrize("name", ["a", "d1_sparse"])
def test_misaligned_image_refuses_the_row_path(name):
    """case j: the gradient image one float into a larger buffer -- no block takes the 16-byte row path"""
    cs = O.case(name)
    c = O.path_census(cs["points"], cs["radii"], cs["rs"], cs["go"], cs["first"], cs["num"], visible=cs["visible"],
                      aligned=False)
    assert c["dense_blocks"] == 0 and c["scan_blocks"] > 0


def test_census_of_a_zero_gradient():
    """case i: no flagged super block -- every point is light, the heavy list stays empty"""
    cs = O.case("a")
    c = O.path_census(cs["points"], cs["radii"], cs["rs"], torch.zeros_like(cs["go"]), cs["first"], cs["num"],
                      visible=cs["visible"])
    assert c["heavy"] == 0 and c["light_zero"] > 0 and c["heavy_strides"] == 0
