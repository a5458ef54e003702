"""The anisotropic and the invariant splat variance (Vrk_isotropic=False / Vrk_invariant=True) on the GPU, against the
reference's own _get_per_point_info (tests/golden/vrk_*.npz: float64 = truth, float32 = yardstick; tests/vrk_util.py).

Figures measured on an MI355X are in DESIGN.md 3.4b."""
import pytest
import torch

import vrk_util as VU

pytestmark = pytest.mark.gpu

MODES = {"anisotropic": dict(Vrk_isotropic=False), "invariant": dict(Vrk_invariant=True), "isotropic": dict()}


def splatter(mode, S=64, K=8, **kw):
    from iso_points_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    return SurfaceSplatting(raster_settings=PointsRasterizationSettings(image_size=S, points_per_pixel=K, **MODES[mode]), **kw)


def on_device(g, dev):
    from iso_points_amd.levelset_sampling import with_host_lengths
    num = with_host_lengths(g["num"].long().to(dev), g["num"].tolist())
    fl = [at for at, _ in VU.view_slices(g["num"])]
    first = with_host_lengths(torch.tensor(fl, dtype=torch.int64, device=dev), fl)
    return g["points"].to(dev), g["normals"].to(dev), first, num, g["views"].to(dev), g["projs"].to(dev)


def ndc_truth(g):
    from oracle import splat_oracle as SO
    return torch.cat([SO.transform_to_ndc(g["points"][at:at + n].double(), g["views"][v].double(), g["projs"][v].double())
                      for v, (at, n) in enumerate(VU.view_slices(g["num"]))])


@pytest.mark.parametrize("scene", VU.SCENES)
def test_anisotropic_per_point_info_matches_the_reference(dev, scene):
    g = VU.load(scene)
    ss = splatter("anisotropic", S=g["image_size"], frnn_radius=g["frnn_radius"])
    dbg = {}
    ndc, info = ss.per_point_info(*on_device(g, dev), debug=dbg)
    pmax = int(g["num"].max())
    assert torch.equal(dbg["knn_idx"].cpu()[:, :pmax], g["knn_idx"].long())          # the kNN index, exactly
    assert not hasattr(ss, "_knn_idx")
    assert ss._Vrk_h is None
    keep = VU.well_posed_rows(g)
    print("%s: %d of %d rows with an ill-posed normal left out" % (scene, int((~keep).sum()), keep.numel()))
    for k in ("radii", "ellipse_params", "scaler"):
        VU.judge("%s anisotropic %s" % (scene, k), info[k].cpu(), g["aniso_%s_f64" % k], g["aniso_%s_f32" % k], keep)
    assert torch.equal(info["cutoff_threshold"].cpu(), g["aniso_cutoff_threshold_f32"])
    e = VU.row_err(ndc.cpu(), ndc_truth(g))
    print("%s ndc: max rel err %.3g" % (scene, e.max()))
    assert e.max().item() < 1e-6
    assert all(not t.requires_grad for t in info.values())


@pytest.mark.parametrize("scene", VU.SCENES)
def test_invariant_per_point_info_matches_the_reference(dev, scene):
    g = VU.load(scene)
    ss = splatter("invariant", S=g["image_size"], frnn_radius=g["frnn_radius"])
    ndc, info = ss.per_point_info(*on_device(g, dev))
    h = ss._Vrk_h.cpu()
    ulp = VU.ulp_distance(h, g["invariant_h_f32"])
    print("%s invariant h per view %s; distance to the float32 reference: %d ulp; to the float64 one: %.3g relative"
          % (scene, sorted(set(h.tolist())), int(ulp.max()), ((h.double() - g["invariant_h_f64"]).abs() / g["invariant_h_f64"]).max()))
    assert int(ulp.max()) <= 1
    for k in ("radii", "ellipse_params", "scaler"):
        VU.judge("%s invariant %s" % (scene, k), info[k].cpu(), g["invariant_%s_f64" % k], g["invariant_%s_f32" % k])
    assert torch.equal(info["cutoff_threshold"].cpu(), g["invariant_cutoff_threshold_f32"])
    assert VU.row_err(ndc.cpu(), ndc_truth(g)).max().item() < 1e-6
    # not a cache: another cloud through the same object gets its own h
    g2 = VU.load("cube" if scene == "sphere" else "sphere")
    ss.per_point_info(*on_device(g2, dev))
    assert int(VU.ulp_distance(ss._Vrk_h.cpu(), g2["invariant_h_f32"]).max()) <= 1


def _setup_call(name, dev, g, *front, n_rows=None):
    from iso_points_amd import _lib
    pts, nrm, first, num, views, projs = on_device(g, dev)
    tot = pts.shape[0]
    outs = [torch.empty((tot, w), dtype=torch.float32, device=dev) for w in (3, 3, 1, 2, 1)]
    p = _lib.ptr
    size = (int(g["image_size"]), float(g["sigma"]), float(g["cutoff"]))
    mx = int(g["num"].max())
    if name == "iso_splat_setup_aniso":
        (idx,) = front
        _lib.call(name, p(pts), p(idx), idx.shape[1], p(first), p(num), p(views), p(projs), len(g["num"]), *size,
                  *[p(o) for o in outs], _lib.stream())
    else:
        a, b = front
        _lib.call(name, p(pts), p(a), p(b), p(first), p(num), p(views), p(projs), len(g["num"]), mx, *size,
                  *[p(o) for o in outs], _lib.stream())
    torch.cuda.synchronize()
    return outs


def _padded(g, dev):
    num = g["num"].tolist()
    padded = torch.zeros((len(num), max(num), 3), dtype=torch.float32, device=dev)
    for v, (at, n) in enumerate(VU.view_slices(g["num"])):
        padded[v, :n] = g["points"][at:at + n].to(dev)
    return padded


@pytest.mark.parametrize("scene", VU.SCENES)
def test_layering_identities(dev, scene):
    from iso_points_amd.math_helper import pca_frames
    g = VU.load(scene)
    pts, nrm, first, num, views, projs = on_device(g, dev)
    # (1) the explicit-frame entry fed the isotropic kernel's own frame and (., h, h) = the isotropic entry, to 2 ulp, on
    # the scene's own (general) normals.  The frame is the kernel's, to the bit: iso_splat_tangent_frame exports it.
    from iso_points_amd import _lib
    h = (torch.rand(pts.shape[0], generator=torch.Generator().manual_seed(3)) * 9e-3 + 1e-4).to(dev)
    curv = torch.stack([torch.zeros_like(h), h, h], dim=-1).contiguous()
    u, v = torch.empty_like(nrm), torch.empty_like(nrm)
    _lib.call("iso_splat_tangent_frame", _lib.ptr(nrm), nrm.shape[0], _lib.ptr(u), _lib.ptr(v), _lib.stream())
    hu, hv = VU.kernel_tangent_frame(g["normals"])
    print("%s: exported frame vs its host restatement: max |du| %.3g, |dv| %.3g; |u| - 1 max %.3g, |<u, n>| max %.3g"
          % (scene, (u.cpu() - hu).abs().max(), (v.cpu() - hv).abs().max(), (u.norm(dim=-1) - 1).abs().max(),
             (u * torch.nn.functional.normalize(nrm, dim=-1)).sum(-1).abs().max()))
    assert (u.cpu() - hu).abs().max().item() < 1e-6 and (v.cpu() - hv).abs().max().item() < 1e-6
    frames = torch.stack([nrm, u, v], dim=-1).contiguous()                                     # columns n, u, v
    iso = _setup_call("iso_splat_setup", dev, g, nrm, h)
    vrk = _setup_call("iso_splat_setup_vrk", dev, g, frames, curv)
    for name, a, b in zip(("ndc", "ellipse", "cutoff", "radii", "scaler"), iso, vrk):
        d = int(VU.ulp_distance(a, b).max())
        print("%s: explicit frame (h, h) vs isotropic entry: %s max %d ulp" % (scene, name, d))
        assert d <= 2, (name, d)
    # (2) fused = unfused, bit for bit
    idx = g["knn_idx"].long().to(dev).contiguous()
    curv, fr = pca_frames(_padded(g, dev), num, idx, disambiguate_directions=False)
    rows = torch.cat([torch.arange(n, device=dev) + v * idx.shape[1] for v, n in enumerate(g["num"].tolist())])
    fr_p, curv_p = fr.reshape(-1, 3, 3)[rows].contiguous(), curv.reshape(-1, 3)[rows].contiguous()
    unfused = _setup_call("iso_splat_setup_vrk", dev, g, fr_p, curv_p)
    fused = _setup_call("iso_splat_setup_aniso", dev, g, idx)
    for name, a, b in zip(("ndc", "ellipse", "cutoff", "radii", "scaler"), unfused, fused):
        assert torch.equal(a, b), name
    # (3) the sign of u or v changes no output bit
    for col in (1, 2):
        flipped = fr_p.clone()
        flipped[:, :, col] = -flipped[:, :, col]
        for name, a, b in zip(("ndc", "ellipse", "cutoff", "radii", "scaler"), unfused,
                              _setup_call("iso_splat_setup_vrk", dev, g, flipped, curv_p)):
            assert torch.equal(a, b), (col, name)


def _world(dev, P=6000, seed=44, n_views=3, S=64):
    from splat_util import sphere_scene
    sc = sphere_scene(P, n_views=n_views, S=S, seed=seed)
    projs = torch.stack([v @ sc["proj"] for v in sc["views"]])
    return sc["world_points"].to(dev), sc["world_normals"].to(dev), sc["views"].to(dev), projs.to(dev)


def _chain(ss, clouds, views, projs):
    """filter -> compact -> ONE per_point_info over the whole packed batch -> _C.splat_points, by hand, as the reference
    does it (rasterizer.py:597-661).  clouds: [(points, normals)]; one cloud is seen by every camera, B clouds by camera b."""
    from iso_points_amd.rasterizer import _C
    from iso_points_amd.levelset_sampling import with_host_lengths
    rs = ss.raster_settings
    N = views.shape[0]
    pf, nf, lens, flags_all = [], [], [], []
    for b, (pts, nrm) in enumerate(clouds):
        vw = views if len(clouds) == 1 else views[b:b + 1]
        flags, off, ln = ss.filter_renderable(pts, nrm, vw)
        pf.append(ss.compact(pts, flags, off, pts.shape[0], sum(ln)))
        nf.append(ss.compact(nrm, flags, off, pts.shape[0], sum(ln)))
        lens += ln
        flags_all.append(flags[:-1].view(vw.shape[0], -1))
    assert len(lens) == N
    fl = [sum(lens[:i]) for i in range(N)]
    num = with_host_lengths(torch.tensor(lens, dtype=torch.int64, device=views.device), lens)
    first = with_host_lengths(torch.tensor(fl, dtype=torch.int64, device=views.device), fl)
    ndc, info = ss.per_point_info(torch.cat(pf), torch.cat(nf), first, num, views, projs)
    out = _C.splat_points(ndc, info["ellipse_params"], info["cutoff_threshold"], info["radii"], first, num,
                          rs.depth_merging_threshold, rs.image_size, int(rs.points_per_pixel))
    return ndc, info, out, (flags_all, first, num), ss._Vrk_h


def _same_as_chain(frags, filt, ss_fwd, chain):
    ndc, info, (idx, zbuf, qv, occ), (flags_all, first, num), h = chain
    assert filt["num_points"].tolist() == num.tolist() and filt["first_idx"].tolist() == first.tolist()
    assert torch.equal(filt["ndc"], ndc)
    for k in VU.KEYS:
        assert torch.equal(filt[k], info[k]), k
    assert torch.equal(frags.idx, idx) and torch.equal(frags.zbuf, zbuf) and torch.equal(frags.qvalue, qv)
    assert torch.equal(frags.occupancy, occ)
    assert bool((frags.idx >= 0).any()) and torch.isfinite(frags.qvalue).all()
    if h is None:
        assert ss_fwd._Vrk_h is None
    else:
        assert torch.equal(ss_fwd._Vrk_h, h)


class _Clouds(object):
    def __init__(self, worlds):
        self.w = worlds

    def __len__(self):
        return len(self.w)

    def points_list(self):
        return [w[0] for w in self.w]

    def normals_list(self):
        return [w[1] for w in self.w]

    def points_packed(self):
        return torch.cat(self.points_list())


@pytest.mark.parametrize("mode", ["anisotropic", "invariant"])
def test_forward_equals_the_chain_one_cloud_three_views(dev, mode):
    pts, nrm, views, projs = _world(dev)
    ss = splatter(mode)
    frags, filt = ss.forward(pts, nrm, cameras=(views, projs))
    chain = _chain(splatter(mode), [(pts, nrm)], views, projs)
    _same_as_chain(frags, filt, ss, chain)
    assert torch.equal(filt["flags"].bool(), chain[3][0][0].bool())
    assert torch.equal(filt["points"], pts[filt["src"]])


@pytest.mark.parametrize("mode", ["anisotropic", "invariant"])
def test_forward_equals_the_chain_one_cloud_ten_views(dev, mode):
    """More than 8 views: forward() works in runs of 8, the reference batches all ten -- the invariant mean's padded length
    is the largest of the ten view clouds."""
    pts, nrm, views, projs = _world(dev, P=5000, seed=9, n_views=10)
    ss = splatter(mode)
    frags, filt = ss.forward(pts, nrm, cameras=(views, projs))
    chain = _chain(splatter(mode), [(pts, nrm)], views, projs)
    assert len(set(chain[3][2].tolist())) > 1                              # ragged view clouds
    _same_as_chain(frags, filt, ss, chain)


@pytest.mark.parametrize("mode", ["anisotropic", "invariant"])
def test_forward_equals_the_chain_batch_of_unequal_clouds(dev, mode):
    """B clouds with B cameras: every job of forward() holds one view, the reference's padded tensor holds all of them.
    The cube-sized clouds (0.3 x the sphere scene) keep the mean bandwidth between the clamps, so that h shows which
    padded length was used: the largest cloud's own mean, the others pulled down by their padded rows."""
    worlds = [_world(dev, P=P, seed=s, n_views=3) for P, s in ((6000, 5), (3500, 6), (4800, 7))]
    views, projs = worlds[0][2], worlds[0][3]
    clouds = [((0.35 * w[0]).contiguous(), w[1]) for w in worlds]
    ss = splatter(mode)
    frags, filt = ss.forward(_Clouds(clouds), cameras=(views, projs))
    chain = _chain(splatter(mode), clouds, views, projs)
    assert len(set(chain[3][2].tolist())) == 3
    _same_as_chain(frags, filt, ss, chain)
    if mode == "invariant":
        hs = [float(chain[4][int(f)]) for f in chain[3][1].tolist()]
        print("invariant h of the three clouds (rows %s): %s" % (chain[3][2].tolist(), hs))
        assert len(set(hs)) > 1
        # ... and it is NOT what each cloud would get on its own
        own = splatter(mode)
        _chain(own, clouds[1:2], views[1:2], projs[1:2])
        assert float(own._Vrk_h[0]) != hs[1]


@pytest.mark.parametrize("mode", ["anisotropic", "invariant"])
def test_backward_reaches_the_world_points(dev, mode):
    """The per-point info is detached in every mode, so the gradient of an image loss reaches the world points through the
    NDC rows alone: forward()'s graph = the default-mode machinery (_WorldToRows -> EllipticalRasterizer, whose backward is
    _C._backward) applied by hand to the same radii / ellipses."""
    from iso_points_amd.rasterizer import PackedClouds, _WorldToRows, composite, gather_with_neg_idx, rasterize_elliptical_points
    from iso_points_amd.rasterizer import PointFragments
    pts, nrm, views, projs = _world(dev)
    col = (0.5 * (nrm + 1)).contiguous()
    target = torch.rand((views.shape[0], 64, 64, 4), generator=torch.Generator().manual_seed(1)).to(dev)

    ss = splatter(mode)
    x = pts.clone().requires_grad_(True)
    frags, filt = ss.forward(x, nrm, cameras=(views, projs), features=col)
    img = composite(frags, filt["scaler"], filt["features"])
    ((img - target) ** 2).sum().backward()
    g_fwd = x.grad.clone()
    assert torch.isfinite(g_fwd).all() and float(g_fwd.abs().max()) > 0

    ss2 = splatter(mode)
    rs = ss2.raster_settings
    fr = ss2.front_filtered(pts, nrm, views, projs, features=col)
    y = pts.clone().requires_grad_(True)
    rows = _WorldToRows.apply(y, fr["ndc"], views, projs, fr["mask"], fr["src"], fr["first_idx"], fr["num_points"])
    idx, zbuf, qv, occ = rasterize_elliptical_points(
        PackedClouds(rows, fr["first_idx"], fr["num_points"]), fr["ellipse_params"], fr["cutoff_threshold"], fr["radii"],
        depth_merging_threshold=rs.depth_merging_threshold, image_size=rs.image_size, points_per_pixel=int(rs.points_per_pixel),
        bin_size=rs.bin_size, max_points_per_bin=rs.max_points_per_bin, radii_backward_scaler=rs.radii_backward_scaler,
        clip_pts_grad=rs.clip_pts_grad)
    frags2 = PointFragments(idx, zbuf, qv, gather_with_neg_idx(fr["scaler"], idx), occ)
    img2 = composite(frags2, fr["scaler"], fr["features"])
    assert torch.equal(img2, img)
    ((img2 - target) ** 2).sum().backward()
    assert torch.equal(y.grad, g_fwd)


def test_default_mode_is_untouched_by_the_other_modes(dev):
    """No state leaks between modes (_Vrk_h, grids, pair capacities): the default mode gives the same bits on a fresh
    object and on one that has served both non-default modes."""
    from iso_points_amd.rasterizer import PointsRasterizationSettings
    pts, nrm, views, projs = _world(dev)
    g = VU.load("sphere")
    args = on_device(g, dev)

    def default_run(ss):
        ndc, info = ss.per_point_info(*args)
        h = ss._Vrk_h.clone()
        frags, filt = ss.forward(pts, nrm, cameras=(views, projs))
        return [ndc, h, ss._Vrk_h] + [info[k] for k in VU.KEYS] + [filt[k] for k in VU.KEYS] + \
            [filt["ndc"], frags.idx, frags.zbuf, frags.qvalue, frags.occupancy]

    fresh = default_run(splatter("isotropic"))
    used = splatter("isotropic")
    for mode in ("anisotropic", "invariant"):
        used.raster_settings = PointsRasterizationSettings(image_size=64, points_per_pixel=8, **MODES[mode])
        used.per_point_info(*args)
        used.forward(pts, nrm, cameras=(views, projs))
    used.raster_settings = PointsRasterizationSettings(image_size=64, points_per_pixel=8)
    again = default_run(used)
    for i, (a, b) in enumerate(zip(fresh, again)):
        assert torch.equal(a, b), i
    # ... and the default set-up is the one the existing fixture pins
    from splat_util import sphere_scene
    sc = sphere_scene(3000, n_views=3, S=64, seed=21)
    assert torch.equal(fresh[1].cpu(), sc["h"])


def test_refusals(dev):
    from iso_points_amd.dist import IsoCycle
    from iso_points_amd.rasterizer import PointsRasterizationSettings
    g = VU.load("cube")
    pts, nrm, first, num, views, projs = on_device(g, dev)
    from iso_points_amd.levelset_sampling import with_host_lengths
    few = with_host_lengths(torch.tensor([8], dtype=torch.int64, device=dev), [8])
    zero = with_host_lengths(torch.tensor([0], dtype=torch.int64, device=dev), [0])
    with pytest.raises(ValueError, match="neighborhood_size"):
        splatter("anisotropic").per_point_info(pts[:8].contiguous(), nrm[:8].contiguous(), zero, few, views[:1], projs[:1])
    nine = with_host_lengths(torch.tensor([9], dtype=torch.int64, device=dev), [9])
    _, info = splatter("anisotropic").per_point_info(pts[:9].contiguous(), nrm[:9].contiguous(), zero, nine, views[:1], projs[:1])
    assert torch.isfinite(info["radii"]).all()
    for mode in ("anisotropic", "invariant"):
        rs = PointsRasterizationSettings(image_size=64, points_per_pixel=8, **MODES[mode])
        with pytest.raises(NotImplementedError, match="out of scope"):
            IsoCycle(None, pts, views, projs, raster_settings=rs)
        with pytest.raises(NotImplementedError, match="filtered route"):
            splatter(mode).front(pts, nrm, views, projs)


@pytest.mark.parametrize("mode", ["anisotropic", "invariant"])
def test_full_size_each_mode_twice(dev, mode):
    """1 M points x 4 views (BASELINE.json configs[2]'s shape): two runs give identical bits, everything is finite, no row
    was dropped."""
    from oracle import splat_oracle as SO
    P, S, K, N = 1000000, 512, 8, 4
    gen = torch.Generator().manual_seed(0)
    pts = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).to(dev)
    nrm = pts.clone()
    views = torch.stack([SO.look_at_view(5.0, 20.0, 90.0 * i) for i in range(N)]).to(dev)
    projs = views @ SO.perspective(30.0).to(dev)
    ss = splatter(mode, S=S, K=K)
    runs = []
    for _ in range(2):
        frags, filt = ss.forward(pts, nrm, cameras=(views, projs))
        runs.append([frags.idx, frags.zbuf, frags.qvalue, frags.occupancy, frags.scaler, filt["ndc"]] + [filt[k] for k in VU.KEYS])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for t in runs[0][1:]:
        assert torch.isfinite(t).all()
    assert sum(filt["num_points"].tolist()) == filt["ndc"].shape[0] > P
    ovf = getattr(ss, "_row_overflow", None)
    assert ovf is None or int(ovf.item()) == 0
    assert 0.05 < frags.occupancy.mean().item() < 0.5
