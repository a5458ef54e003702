"""The references of the splat front end (splat_front_oracle.py) against what the suite already pins -- the oracle's
per_point_info / filter_renderable, the packed layout of splat_util.sphere_scene, central differences -- and the table
of the float32 yardstick against float64 over the case list of test_splat_front_gpu.py.  No GPU."""
import pytest
import torch

import splat_front_oracle as FO
from oracle import splat_oracle as SO
from splat_util import sphere_scene

F64 = torch.float64


@pytest.fixture(scope="module")
def scene():
    return sphere_scene(3000, n_views=3, S=64, seed=12)


def test_mask_and_pack_against_the_sphere_scene(scene):
    sc = scene
    for fl in (FO.flags_ref(sc["world_points"], sc["world_normals"], sc["views"]),
               FO.mask64(sc["world_points"], sc["world_normals"], sc["views"])):
        assert torch.equal(fl, sc["keep"])                       # (no point of this scene sits on a threshold)
    bits = FO.mask_bits(sc["keep"])
    assert torch.equal(FO.bits_to_flags(bits, 3), sc["keep"])
    first, num, src = FO.pack_ref(bits, 3)
    assert torch.equal(first, sc["first"]) and torch.equal(num, sc["num"])
    assert torch.equal(sc["world_points"][src.long()], sc["points"])
    assert torch.equal(FO.view_total_ref(num)[:3], num.int()) and not FO.view_total_ref(num)[3:].any()
    # without culling and with a narrow slab
    fl = FO.flags_ref(sc["world_points"], sc["world_normals"], sc["views"], 2.5, 3.0, False)
    for v in range(3):
        assert torch.equal(fl[v], SO.filter_renderable(sc["world_points"], sc["world_normals"], sc["views"][v], 2.5, 3.0, False))
    assert 0 < fl.sum() < fl.numel()


def test_pack_ref_of_hand_made_masks():
    m = torch.tensor([0b101, 0, 0b111, 0b010, 0b100], dtype=torch.int32)
    first, num, src = FO.pack_ref(m, 4)
    assert first.tolist() == [0, 2, 4, 7] and num.tolist() == [2, 2, 3, 0]
    assert src.tolist() == [0, 2, 2, 3, 0, 2, 4] and src.dtype == torch.int32
    first, num, src = FO.pack_ref(torch.zeros(0, dtype=torch.int32), 2)
    assert first.tolist() == [0, 0] and num.tolist() == [0, 0] and src.numel() == 0


def test_thresholds_are_inclusive_for_depth_and_strict_for_the_normal():
    V = torch.eye(4)
    V[3, 2] = 2.0
    pts = torch.tensor([[0.0, 0, -1.0], [0, 0, 98.0], [0, 0, -1.0 - 2.0 ** -22], [0, 0, 98.0 + 2.0 ** -17], [0, 0, 5.0]])
    nrm = torch.tensor([[0.0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [1, 0, 0]])
    for f in (FO.flags_ref, FO.mask64):
        assert f(pts, nrm, V[None])[0].tolist() == [True, True, False, False, False]


def test_setup64_equals_the_oracle_in_float64(scene):
    sc = scene
    s0 = 0
    for v, n in enumerate(sc["num"].tolist()):
        sl = slice(s0, s0 + n)
        M = sc["views"][v] @ sc["proj"]
        t = FO.setup64(sc["points"][sl], sc["normals"][sl], sc["h"][sl], sc["views"][v], M, 64)
        ref = SO.per_point_info(sc["points"][sl], sc["normals"][sl], sc["h"][sl], M, 64, dtype=F64)
        for k in ("ellipse_params", "radii", "scaler"):
            assert torch.equal(t[k], ref[k]), k
        ndc = SO.transform_to_ndc(sc["points"][sl].double(), sc["views"][v].double(), M.double())
        assert torch.equal(t["ndc"], ndc)
        assert (t["ndc"].float() - sc["ndc"][sl]).abs().max() < 1e-6
        s0 += n


@pytest.mark.parametrize("cam", FO.CAMERAS)
@pytest.mark.parametrize("normals", FO.NORMALS)
def test_kernel_statements_in_float64_equal_setup64(cam, normals):
    """The restatement of splat_setup_point evaluated in float64 (expansion of det G, both radii statements, the
    kernel's helper axis) against the reference's statements in float64: the restatement is the same function, and the
    result does not depend on the helper axis."""
    V, M = FO.camera(cam)
    pts, nrm = FO.case_cloud(normals, V, seed=3, P=500)
    for S, h in ((64, 0.01), (1040, 5e-5), (1040, 0.01)):
        hk = torch.full((pts.shape[0],), h)
        truth = FO.setup64(pts, nrm, hk, V, M, S)
        # grazing rows: cond(G) up to ~1e4, so the textbook float64 statements themselves hold ~1e-12
        for form in ("den", "g"):
            got = FO._setup_kernel_form(pts, nrm, hk, V, M, S, 1.0, 1.0, F64, form)
            err = FO.row_errors(got, truth)
            for k, e in err.items():
                assert e.max().item() < 1e-9, (form, k, e.max().item())
        # another valid frame (the oracle's argmin helper axis, rotated by 0.3 rad in the tangent plane)
        Sk = SO.tangent_frame(nrm.double())
        c, s = torch.cos(torch.tensor(0.3, dtype=F64)), torch.sin(torch.tensor(0.3, dtype=F64))
        fr = torch.stack([c * Sk[:, 0] + s * Sk[:, 1], -s * Sk[:, 0] + c * Sk[:, 1]])
        got = FO._setup_kernel_form(pts, nrm, hk, V, M, S, 1.0, 1.0, F64, "g", frame=fr)
        for k, e in FO.row_errors(got, truth).items():
            assert e.max().item() < 1e-9, ("rotated frame", k, e.max().item())


def test_radii_identity():
    """4ac - b^2 = 4 / det G, so radii = (sqrt(g00 cutoff), sqrt(g11 cutoff)): against setup64's statement."""
    V, M = FO.camera("perspective")
    pts, nrm = FO.case_cloud("grazing", V, seed=5)
    hk = torch.full((pts.shape[0],), 0.01)
    for cutoff in (1.0, 2.5):
        truth = FO.setup64(pts, nrm, hk, V, M, 1040, cutoff=cutoff)
        el = truth["ellipse_params"]
        a, b, c = el[:, 0], el[:, 1], el[:, 2]
        det_g = 4.0 / (4 * a * c - b * b)
        g00, g11 = c * det_g, a * det_g
        r = torch.stack([torch.sqrt(g00 * cutoff), torch.sqrt(g11 * cutoff)], -1)
        assert ((r - truth["radii"]).abs() / truth["radii"]).max().item() < 1e-11


def test_points_backward64_against_central_differences():
    g = torch.Generator().manual_seed(2)
    P, N = 300, 3
    pts = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    views = torch.stack([SO.look_at_view(3.0 + 0.3 * i, 10.0 * i, 100.0 * i) for i in range(N)])
    projs = torch.stack([v @ SO.perspective(30.0) for v in views])
    flags = torch.rand(N, P, generator=g) < 0.5
    flags[:, 7] = False
    first, num, src = FO.pack_ref(flags, N)
    gn = torch.randn(int(num.sum()), 3, generator=g)
    grad, scale = FO.points_backward64(pts, views, projs, flags, first, src, gn)
    assert (grad[7] == 0).all() and scale[7] == 0 and (scale[flags.any(0)] > 0).all()

    def loss(x):
        tot = 0.0
        for v in range(N):
            rows = slice(int(first[v]), int(first[v] + num[v]))
            ph = torch.cat([x[flags[v]], torch.ones(int(num[v]), 1, dtype=F64)], 1)
            clip = ph @ projs[v].double()
            ndc = torch.stack([clip[:, 0] / clip[:, 3], clip[:, 1] / clip[:, 3], (ph @ views[v].double())[:, 2]], 1)
            tot = tot + (ndc * gn[rows].double()).sum()
        return tot

    x0, eps = pts.double(), 1e-6
    for i in (0, 7, 150, 299):
        for j in range(3):
            d = torch.zeros(P, 3, dtype=F64)
            d[i, j] = eps
            fd = (loss(x0 + d) - loss(x0 - d)) / (2 * eps)
            assert abs(fd - grad[i, j]) <= 1e-7 * max(scale[i].item(), 1e-30) + 1e-9, (i, j, fd, grad[i, j])
    g32 = FO.points_backward32(pts, views, projs, flags, first, src, gn)
    e = (g32.double() - grad).abs().amax(-1) / scale.clamp(min=1e-300)
    assert e.max().item() < 1e-6 and (g32[7] == 0).all()


def test_vrk_h_ref():
    d = torch.full((2, 5, 7), -1.0)
    d[0, 0] = torch.tensor([0, 1e-3, 2e-3, 3e-3, 4e-3, 5e-3, 6e-3])          # 6 hits
    d[0, 1, :4] = torch.tensor([0, 1e-5, 2e-5, 3e-5])                        # 3 hits -> lower clamp
    d[0, 2, 0] = 0.0                                                         # no hit but itself
    d[0, 3] = torch.tensor([0, 0.5, 0.1, 0.2, 0.3, 0.4, 0.45])               # upper clamp
    d[1, 0] = torch.tensor([0.0, 1, 1, 1, 1, 1, 1])
    h = FO.vrk_h_ref(d, torch.tensor([4, 3]), cloud_num=torch.tensor([9, 3]))    # cloud 1: the 1e-3 branch
    f = lambda x: torch.tensor(x, dtype=torch.float32).item()                # noqa: E731
    assert h.tolist() == [f(3e-3), f(5e-5), f(5e-5), f(0.01), f(5e-4), f(5e-4), f(5e-4)]
    # the oracle's own statement on a real cloud
    g = torch.Generator().manual_seed(1)
    pts = torch.rand(1, 400, 3, generator=g) * 0.5
    num = torch.tensor([400])
    from oracle.iso_oracle import frnn_grid_points
    sq = frnn_grid_points(pts, pts, num, num, K=7, r=0.05)[0]
    assert (sq == -1).any()
    assert torch.equal(FO.vrk_h_ref(sq, num), SO.vrk_h(pts, num, 0.05))


def test_float32_yardstick_table():
    """setup32 (the kernel's statements, float32) and the reference's float32 arithmetic against setup64 over the case
    list of the GPU accuracy rule: printed; setup32 is finite everywhere, h = 0 included."""
    worst = {k: [0.0, 0.0, 0.0] for k in FO.OUTPUTS}
    cams = {c: FO.camera(c) for c in FO.CAMERAS}
    for name, cam, normals, S, h in FO.setup_cases():
        V, M = cams[cam]
        pts, nrm = FO.case_cloud(normals, V, seed=S)
        hk = torch.full((pts.shape[0],), h)
        truth = FO.setup64(pts, nrm, hk, V, M, S)
        forms = (FO.setup32(pts, nrm, hk, V, M, S, radii_form="den"), FO.setup32(pts, nrm, hk, V, M, S, radii_form="g"),
                 FO.reference32(pts, nrm, hk, V, M, S))
        for f in forms[:2]:
            for k in FO.OUTPUTS:
                assert torch.isfinite(f[k]).all(), (name, k)
        errs = [FO.row_errors(f, truth) for f in forms]
        line = []
        for k in FO.OUTPUTS:
            m = [torch.nan_to_num(e[k], nan=float("inf")).max().item() for e in errs]
            worst[k] = [max(a, b) for a, b in zip(worst[k], m)]
            line.append("%s %.2e/%.2e/%.2e" % (k[:7], *m))
        print("%-36s %s" % (name, "  ".join(line)))
    print("max error against float64 (setup32 with radii from 4ac - b^2 / setup32 with radii from g / float32 reference):")
    for k in FO.OUTPUTS:
        print("  %-15s %.3g / %.3g / %.3g" % (k, *worst[k]))
    # what the yardstick is for: the expansion of det G keeps the ellipse at float32 rounding where the textbook
    # determinant does not (the figures are properties of the formulas, not of a kernel)
    assert worst["ellipse_params"][0] < 5e-5 < worst["ellipse_params"][2]
    assert worst["radii"][1] < 5e-6 < worst["radii"][0]


def test_a_zero_normal_is_finite():
    V, M = FO.camera("perspective")
    pts, _ = FO.case_cloud("radial", V, seed=1, P=16)
    for f in (FO.setup32, FO.setup64):
        out = f(pts, torch.zeros_like(pts), torch.full((16,), 0.01), V, M, 64)
        for k in FO.OUTPUTS:
            assert torch.isfinite(out[k]).all(), k
        assert (out["scaler"] == 0).all()
