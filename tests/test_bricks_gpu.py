"""Brick grid + fused neighbour kernels (include/isopoints.h section E) against the stand-alone
FRNN / repulsion / bandwidth path (itself pinned to the oracle and the reference goldens) and
against the oracle directly: bit-exact neighbour lists and distances, bit-exact moves for the same
inv_sigma, bit-exact h."""
import pytest
import torch

from util import sphere_cloud

pytestmark = pytest.mark.gpu


def _clouds():
    out = {}
    for P in (1, 2, 9, 10, 300, 5000, 100000):
        out["sphere%d" % P] = sphere_cloud(P, seed=100 + P)[0]
    p = sphere_cloud(4000, seed=7)[0]
    p[100:140] = p[50:90]                                   # exact duplicates: ties at d2 = 0 and beyond
    out["duplicates"] = p
    p = sphere_cloud(6000, seed=8)[0]
    p[:5] = torch.tensor([[3.0, 0, 0], [0, -2.5, 0], [0, 0, 4.0], [2, 2, 2], [-3, 1, 0]])   # isolated outliers
    out["outliers"] = p
    g = torch.Generator().manual_seed(9)
    p = torch.rand(20000, 3, generator=g)
    p[:, 2] = 0.25                                          # flat patch: dense fine cells, empty bricks around
    out["plane"] = p
    p = torch.rand(3000, 3, generator=g) * 1e-3
    p[0] = torch.tensor([1.0, 1.0, 1.0])                    # one far point: the grid cannot be fine (overflow bricks)
    out["clump"] = p
    # massive exact distance ties
    out["lattice"] = torch.stack(torch.meshgrid(*([torch.arange(16.0)] * 3), indexing="ij"), -1).view(-1, 3) * 0.05
    return out


CLOUDS = _clouds()


# the full cloud list at the list sizes the callers use, then every other K + 1 in 2..13 on a reduced list, so that each of
# k_brick_resample<8|10|12|16> (K + 1 in 2..5 | 9 | 6..8 | 10..13) runs on both sides of its boundaries
_FUSED_CASES = [(k, n) for n in sorted(CLOUDS) for k in (8, 4, 12)] + \
    [(k, n) for k in (1, 5, 6, 7, 9, 10, 11) for n in ("sphere300", "sphere5000", "duplicates", "lattice", "clump")]


@pytest.mark.parametrize("knn_k,name", _FUSED_CASES, ids=["%d-%s" % c for c in _FUSED_CASES])
def test_resample_fused_equals_standalone(dev, name, knn_k):
    from iso_points_amd import _lib, frnn
    from iso_points_amd.bricks import BrickGrid, resample_fused
    from iso_points_amd.levelset_sampling import UniformProjection, cloud_diag, full_lengths
    pts = CLOUDS[name].to(dev).contiguous()
    P = pts.shape[0]
    g = torch.Generator().manual_seed(5)
    nrm = (CLOUDS[name] + 0.1 * torch.randn(P, 3, generator=g)).to(dev).contiguous()
    grid = BrickGrid(P, dev).build(pts, nrm, knn_k=knn_k)
    out, idx, d2 = resample_fused(grid, knn_k + 1, want_idx=True)
    hdr = grid.header()
    # stand-alone path with the radius / inv_sigma the grid derived (its own sqrt(diag/P)*K may
    # differ from torch's by an ulp)
    num = full_lengths(pts[None])
    dists, idxs, _, _ = frnn.frnn_grid_points(pts[None], pts[None], num, num, K=knn_k + 1, r=hdr["r"])
    assert torch.equal(idx, idxs[0, :, 1:]), "neighbour lists differ (%s)" % hdr
    assert torch.equal(d2, dists[0, :, 1:])
    inv_sigma = torch.tensor([hdr["inv_sigma"]], dtype=torch.float32, device=dev)
    proj = UniformProjection(knn_k=knn_k)
    ref = proj.repulsion_step(pts[None], nrm[None], idxs[..., 1:], inv_sigma)[0]
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)) or torch.equal(out.isnan(), ref.isnan()) and \
        torch.equal(out.nan_to_num(), ref.nan_to_num())
    # the derived radius / inv_sigma against the reference formulas (levelset_sampling.py:129-131,:256)
    diag = cloud_diag(pts[None])[0].item()
    if P > 1 and diag > 0:
        assert abs(hdr["r"] - (diag / P) ** 0.5 * knn_k) <= 1e-6 * hdr["r"]
        assert abs(hdr["inv_sigma"] - P / diag) <= 1e-6 * hdr["inv_sigma"]
    if name.startswith("sphere") and P >= 5000 and knn_k <= 8:
        assert hdr["overflow_bricks"] == 0, hdr


def test_resample_fused_vs_oracle(dev):
    """Directly against the CPU restatement (levelset_sampling.py:110-140,254-284)."""
    from oracle import iso_oracle as O
    from iso_points_amd.bricks import BrickGrid, resample_fused
    P, K = 4000, 8
    p = sphere_cloud(P, seed=31)
    g = torch.Generator().manual_seed(32)
    normals = p + 0.1 * torch.randn(1, P, 3, generator=g)
    r = O.search_radius(p, torch.tensor([P]), K)
    _, idxs, _, _ = O.frnn_grid_points(p, p, K=K + 1, r=r)
    diag = (p.view(-1, 3).max(0).values - p.view(-1, 3).min(0).values).norm().item()
    ref = O.repulsion_step(p, torch.nn.functional.normalize(normals, dim=-1), idxs[..., 1:], torch.tensor([P]) / diag)
    grid = BrickGrid(P, dev).build(p[0].to(dev).contiguous(), normals[0].to(dev).contiguous(), knn_k=K)
    out, idx, _ = resample_fused(grid, K + 1, want_idx=True)
    assert torch.equal(idx.cpu(), idxs[0, :, 1:])
    assert ((out.cpu() - ref[0]).abs().max() / (ref[0] - p[0]).abs().max()).item() < 1e-5


def test_fixed_radius_and_tail(dev):
    """A radius much larger than the fine cell: most queries are finished by the ring walk."""
    from iso_points_amd import frnn
    from iso_points_amd.bricks import BrickGrid, resample_fused
    from iso_points_amd.levelset_sampling import full_lengths
    pts = sphere_cloud(3000, seed=77)[0].to(dev).contiguous()
    P = pts.shape[0]
    grid = BrickGrid(P, dev).build(pts, pts, radius=0.5, knn_k=8, cell_scale=0.5)   # tiny cells: K-th beyond them
    out, idx, d2 = resample_fused(grid, 9, want_idx=True)
    num = full_lengths(pts[None])
    dists, idxs, _, _ = frnn.frnn_grid_points(pts[None], pts[None], num, num, K=9, r=0.5)
    assert grid.header()["tail"] > 0
    assert torch.equal(idx, idxs[0, :, 1:]) and torch.equal(d2, dists[0, :, 1:])


@pytest.mark.parametrize("P,n_views", [(1, 1), (6, 2), (400, 3), (20000, 4), (120000, 4), (3000, 8)])
def test_h_fused_equals_standalone(dev, P, n_views):
    """h of every (view, renderable point) = the K = 7 query of the filtered view cloud + vrk_h."""
    from iso_points_amd.bricks import BrickGrid, H_CELL_SCALE, splat_h_fused, view_mask
    from iso_points_amd.cameras import look_at_view
    from iso_points_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    from iso_points_amd.levelset_sampling import with_host_lengths
    pts = torch.nn.functional.normalize(sphere_cloud(P, seed=11)[0], dim=-1).to(dev).contiguous()
    nrm = pts.clone()
    views = torch.stack([look_at_view(3.0, 20.0, 360.0 / n_views * i) for i in range(n_views)]).to(dev).contiguous()
    ss = SurfaceSplatting(raster_settings=PointsRasterizationSettings(image_size=64))
    flags, off, lens = ss.filter_renderable(pts, nrm, views)
    tot = sum(lens)
    mask, cnt = view_mask(pts, nrm, views)
    assert cnt[:n_views].tolist() == lens
    fl = flags[:-1].view(n_views, P)
    assert torch.equal(((mask[None] >> torch.arange(n_views, device=dev)[:, None]) & 1).int(), fl)
    grid = BrickGrid(P, dev).build(pts, nrm, payload=mask, radius=ss.frnn_radius, cell_scale=H_CELL_SCALE)
    h = splat_h_fused(grid, mask, cnt, n_views)
    if tot == 0:
        return
    first = [sum(lens[:i]) for i in range(n_views)]
    num = with_host_lengths(torch.tensor(lens, dtype=torch.int64, device=dev), lens)
    fst = with_host_lengths(torch.tensor(first, dtype=torch.int64, device=dev), first)
    pts_f = ss.compact(pts, flags, off, P, tot)
    nrm_f = ss.compact(nrm, flags, off, P, tot)
    ss.per_point_info(pts_f, nrm_f, fst, num, views, views)
    ref = ss._Vrk_h
    got = torch.cat([h[v][fl[v].bool()] for v in range(n_views)])
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def test_h_fused_sparse_views(dev):
    """Clouds whose K-th neighbour lies far outside the staged block (ring walk), and a view with
    fewer than 7 renderable points (the reference's 1e-3 branch)."""
    from iso_points_amd.bricks import BrickGrid, splat_h_fused, view_mask
    from iso_points_amd.cameras import look_at_view
    from iso_points_amd.rasterizer import PointsRasterizationSettings, SurfaceSplatting
    from iso_points_amd.levelset_sampling import with_host_lengths
    g = torch.Generator().manual_seed(3)
    pts = torch.nn.functional.normalize(torch.randn(500, 3, generator=g), dim=-1)
    nrm = pts.clone()
    nrm[5:] = -nrm[5:] * torch.tensor([1.0, 1.0, 1.0])       # most normals flipped: few points survive culling
    pts, nrm = pts.to(dev).contiguous(), nrm.to(dev).contiguous()
    views = torch.stack([look_at_view(3.0, 10.0, 120.0 * i) for i in range(3)]).to(dev).contiguous()
    ss = SurfaceSplatting(raster_settings=PointsRasterizationSettings(image_size=64))
    flags, off, lens = ss.filter_renderable(pts, nrm, views)
    mask, cnt = view_mask(pts, nrm, views)
    grid = BrickGrid(500, dev).build(pts, nrm, payload=mask, radius=ss.frnn_radius, cell_scale=0.3)
    h = splat_h_fused(grid, mask, cnt, 3)
    tot = sum(lens)
    first = [sum(lens[:i]) for i in range(3)]
    num = with_host_lengths(torch.tensor(lens, dtype=torch.int64, device=dev), lens)
    fst = with_host_lengths(torch.tensor(first, dtype=torch.int64, device=dev), first)
    ss.per_point_info(ss.compact(pts, flags, off, 500, tot), ss.compact(nrm, flags, off, 500, tot), fst, num, views,
                      views)
    fl = flags[:-1].view(3, 500).bool()
    got = torch.cat([h[v][fl[v]] for v in range(3)])
    assert torch.equal(got, ss._Vrk_h)
    assert grid.header()["tail_h"] > 0
