"""iso_points_amd.point_processing.knn_others and iso_points_amd.loss.surface_losses / ProjectionLoss / RepulsionLoss on
the GPU against the float64 oracle of tests/surface_loss_oracle.py (checked against itself in test_surface_loss_cpu.py).

The sweeps are compared with the oracle fed the GPU's own neighbour lists (the lists are compared with the brute force
separately).  Bound for every entry: |got - ref| <= A, nothing relative; A is 4 x the largest error of the oracle's float32
run against its float64 run on the inputs of the test at hand, that error taken as at least half a float32 step at the
largest reference entry (tests/test_pfsign_gpu.py has the reasoning).  A never comes from the kernel.  Every test prints
the errors it measures.

The ball test d_k > 2 fs d_0 is a hard threshold: a row is compared only where no d_k / (2 fs d_0) lies within 1e-5 of 1 in
float64, and at most 1 % of the rows may be left out.  The inputs must keep min sum_k W >= 1e-12 (the weighted mean of the
repulsion is then well conditioned); the seeds below do.  Neighbour indices are compared as sets, on the rows whose K-th
and (K+1)-th float64 distances differ by more than 1e-5 relative."""
import functools

import pytest
import torch

import surface_loss_oracle as O

pytestmark = pytest.mark.gpu

INF = float("inf")


# ------------------------------------------------------------------------------------------------ the nearest others
@functools.lru_cache(maxsize=None)
def _cloud(P, seed):
    return O.cloud(P, seed)


def _assert_lists(dists, idx, points, K, what):
    """GPU lists of one cloud (L,K) against the float64 brute force."""
    L = points.shape[0]
    ref_d, ref_i = O.knn_others(points, K, extra=1 if L > K + 1 else 0)
    assert idx.dtype == torch.int64 and dists.dtype == torch.float32
    assert not (idx == torch.arange(L)[:, None]).any(), "%s: a point is its own neighbour" % what
    assert (dists[:, 1:] >= dists[:, :-1]).all()
    # fl(a - b) of float32 inputs is within 2^-24 relative, its square within 3, the sum of three within 5: 6 * 2^-24
    err = ((dists.double() - ref_d[:, :K]).abs() / ref_d[:, :K]).max().item()
    print("%s: worst relative distance error %.3g (bound %.3g)" % (what, err, 6 * 2.0 ** -24))
    assert err <= 6 * 2.0 ** -24
    clear = torch.ones(L, dtype=torch.bool)
    if ref_d.shape[1] > K:
        clear = (ref_d[:, K] - ref_d[:, K - 1]) > 1e-5 * ref_d[:, K]
    print("%s: %d of %d rows with a clear K-th neighbour" % (what, int(clear.sum()), L))
    assert clear.float().mean().item() >= 0.99
    same = torch.equal(idx.sort(dim=1).values[clear], ref_i[:, :K].sort(dim=1).values[clear])
    assert same, "%s: neighbour sets differ from the brute force" % what


@pytest.mark.parametrize("K", [5, 31])
def test_knn_others_is_the_wider_query_without_its_first_column(dev, K):
    from iso_points_amd import frnn
    from iso_points_amd.point_processing import knn_others
    pts = _cloud(700, 21)[0][None].to(dev)
    got = knn_others(pts, K=K, return_nn=True)
    d, i, nn, _ = frnn.frnn_grid_points(pts, pts, K=K + 1, r=INF, return_nn=True)
    assert torch.equal(got.dists, d[..., 1:]) and torch.equal(got.idx, i[..., 1:]) and torch.equal(got.knn, nn[..., 1:, :])
    assert (i[..., 0] == torch.arange(700, device=dev)).all()


def test_knn_others_32_against_the_brute_force(dev):
    from iso_points_amd.point_processing import knn_others
    big, small = _cloud(700, 21)[0], _cloud(40, 22)[0]
    one = knn_others(big[None].to(dev), K=32)
    _assert_lists(one.dists[0].cpu(), one.idx[0].cpu(), big, 32, "P = 700")
    batch = torch.full((2, 700, 3), float("nan"))
    batch[0], batch[1, :40] = big, small
    two = knn_others(batch.to(dev), torch.tensor([700, 40], device=dev), K=32, return_nn=True)
    assert torch.equal(two.dists[0], one.dists[0]) and torch.equal(two.idx[0], one.idx[0])
    _assert_lists(two.dists[1, :40].cpu(), two.idx[1, :40].cpu(), small, 32, "batch, the cloud of 40")
    assert (two.idx[1, 40:] == 0).all() and (two.dists[1, 40:] == 0).all() and (two.knn[1, 40:] == 0).all()
    assert torch.equal(two.knn[1, :40].cpu(), small[two.idx[1, :40].cpu()])


def test_knn_others_of_33_points_is_the_whole_cloud(dev):
    from iso_points_amd.point_processing import knn_others
    pts = _cloud(33, 23)[0]
    got = knn_others(pts[None].to(dev), K=32)
    _assert_lists(got.dists[0].cpu(), got.idx[0].cpu(), pts, 32, "P = 33")
    want = torch.stack([torch.cat([torch.arange(i), torch.arange(i + 1, 33)]) for i in range(33)])
    assert torch.equal(got.idx[0].cpu().sort(dim=1).values, want)


# ------------------------------------------------------------------------------------------------ the sweeps
# name -> (lengths, seeds, knn_k)
CASES = {
    "p3000": ((3000,), (31,), 33),
    "batch": ((3000, 400), (31, 32), 33),
    "knn_k9": ((400,), (32,), 9),
    "knn_k2": ((400,), (32,), 2),
    "p33": ((33,), (36,), 33),
}


def _padded(lengths, seeds):
    """(points, normals) (N, max L, 3); the padding is NaN: nothing may read it."""
    P = max(lengths)
    pts = torch.full((len(lengths), P, 3), float("nan"))
    nrm = torch.full((len(lengths), P, 3), float("nan"))
    for b, (L, seed) in enumerate(zip(lengths, seeds)):
        pts[b, :L], nrm[b, :L] = _cloud(L, seed)
    return pts, nrm


def _run(dev, pts, nrm, lengths, **kw):
    """surface_losses with gradients: dict of CPU tensors, padded where the call returns padded."""
    from iso_points_amd.loss import _mollify, surface_losses
    p = pts.to(dev).requires_grad_(True)
    lens = torch.tensor(lengths, device=dev)
    res = surface_losses(p, nrm.to(dev), lens, **kw)
    out = dict(n2=res.normals, idx=res.knn.idx, dists=res.knn.dists, res=res)
    sigma, fs = kw.get("sharpness_sigma", 0.75), kw.get("filter_scale", 2.0)
    out["n1"] = _mollify(nrm.to(dev).contiguous(), res.knn, lens, fs, 1.0 / (sigma * sigma), False)
    for name, loss in (("proj", res.projection), ("rep", res.repulsion)):
        if loss is not None:
            assert loss.shape == (sum(lengths),) and loss.dtype == torch.float32
            out[name] = loss.detach()
            out["g" + name], = torch.autograd.grad(loss.sum(), p, retain_graph=True)
    return {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def _compare(got, pts, nrm, lengths, what, nbr_points=None, **kw):
    """Every cloud of a run against the oracle on the GPU's own lists."""
    first = 0
    for b, L in enumerate(lengths):
        idx, dists = got["idx"][b, :L], got["dists"][b, :L]
        nbr = None if nbr_points is None else nbr_points[b, :L]
        ref = O.sweeps(pts[b, :L], nrm[b, :L], idx, dists, dtype=torch.float64, nbr_points=nbr, **kw)
        f32 = O.sweeps(pts[b, :L], nrm[b, :L], idx, dists, dtype=torch.float32, nbr_points=nbr, **kw)
        keep = ref["margin"] > 1e-5
        print("%s, cloud %d (L = %d, K = %d): %d rows on the ball threshold (nearest margin %.3g), min sum W %.3g, "
              "min sum w %.3g" % (what, b, L, idx.shape[1], int((~keep).sum()), ref["margin"].min().item(),
                                  ref["sum_W"].min().item(), ref["sum_w"].min().item()))
        assert (~keep).float().mean().item() <= 0.01
        assert ref["sum_W"].min().item() >= 1e-12 and ref["sum_w"].min().item() > 0
        rows = {"n1": got["n1"][b, :L], "n2": got["n2"][b, :L]}
        for name in ("proj", "rep"):
            if name in got:
                rows[name] = got[name][first:first + L]
                rows["g" + name] = got["g" + name][b, :L]
        for name, val in rows.items():
            A, err32 = O.tolerance(f32[name][keep], ref[name][keep])
            err = (val.double()[keep] - ref[name].detach()[keep]).abs().max().item()
            print("    %-6s oracle float32 error %.3g -> A %.3g; kernel error %.3g" % (name, err32, A, err))
            assert err <= A, "%s, cloud %d, %s: worst |d| %.3g beyond %.3g" % (what, b, name, err, A)
        for name in ("n1", "n2", "gproj", "grep"):
            if name in got:
                assert (got[name][b, L:] == 0).all(), "%s: %s rows beyond the cloud's length are not zero" % (what, name)
        first += L


@functools.lru_cache(maxsize=None)
def _case(dev, name):
    lengths, seeds, knn_k = CASES[name]
    pts, nrm = _padded(lengths, seeds)
    return pts, nrm, lengths, _run(dev, pts, nrm, lengths, knn_k=knn_k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweeps_match_the_oracle(dev, name):
    pts, nrm, lengths, got = _case(dev, name)
    assert got["idx"].shape[2] == CASES[name][2] - 1
    _compare(got, pts, nrm, lengths, name)


def test_the_batch_computes_each_cloud_as_alone(dev):
    """Per-cloud bandwidth L_b / 2: the first cloud of the batch is the single cloud, bit for bit."""
    _, _, _, one = _case(dev, "p3000")
    _, _, _, two = _case(dev, "batch")
    for k in ("n1", "n2", "gproj", "grep"):
        assert torch.equal(one[k][0], two[k][0]), k
    for k in ("proj", "rep"):
        assert torch.equal(one[k], two[k][:3000]), k


def test_knn_array_source_equals_the_gather_source(dev):
    from iso_points_amd.loss import SurfaceKNN
    from iso_points_amd.point_processing import knn_others
    pts, nrm, lengths, got = _case(dev, "p3000")
    tree = knn_others(pts.to(dev), K=32, return_nn=True)
    assert tree.knn is not None and torch.equal(tree.idx.cpu(), got["idx"])
    again = _run(dev, pts, nrm, lengths, knn=SurfaceKNN(tree.dists, tree.idx, tree.knn, None))
    for k in ("n2", "proj", "rep", "gproj", "grep"):
        assert torch.equal(again[k], got[k]), k
    # columns 1.. of a wider result are read in place: pytorch3d's KNN of knn_k = 33 with its first column dropped
    from iso_points_amd.point_processing import knn_points
    wide = knn_points(pts.to(dev), pts.to(dev), K=32, return_nn=True)
    view = SurfaceKNN(wide.dists[..., 1:], wide.idx[..., 1:], wide.knn[..., 1:, :], None)
    short = _run(dev, pts, nrm, lengths, knn=view)
    full = _run(dev, pts, nrm, lengths, knn_k=32)
    for k in ("n2", "proj", "rep", "gproj", "grep"):
        assert torch.equal(short[k], full[k]), k


def test_lifted_lattice_point(dev):
    """tests/test_surface_loss_cpu.py::test_lifted_lattice_point_projects_to_its_height on the GPU."""
    n, a, h = 9, 1.0 / 16, 1.0 / 64
    lifted = (n // 2) * n + n // 2
    pts, nrm = O.lattice(n, a, lifted, h)
    got = _run(dev, pts[None], nrm[None], (n * n,))
    print("lifted row: proj %.9g against h^2 = %.9g, n2 %s" % (got["proj"][lifted].item(), h * h, got["n2"][0, lifted].tolist()))
    assert abs(got["proj"][lifted].item() - h * h) <= 2e-6 * h * h
    O.assert_plane_normal(got["n2"][0, lifted])
    # dproj/dp = 2 D (-n) with D = -h: 2 h along the normal, the same 13 roundings
    g = got["gproj"][0, lifted].double()
    assert g[0].item() == 0.0 and g[1].item() == 0.0 and abs(g[2].item() - 2 * h) <= 2e-6 * 2 * h


def test_combined_call_equals_the_separate_calls_and_runs_repeat(dev):
    pts, nrm, lengths, both = _case(dev, "batch")
    again = _run(dev, pts, nrm, lengths)
    for k in ("n1", "n2", "proj", "rep", "gproj", "grep", "idx", "dists"):
        assert torch.equal(again[k], both[k]), k
    only_p = _run(dev, pts, nrm, lengths, repulsion=False)
    only_r = _run(dev, pts, nrm, lengths, projection=False)
    assert only_p["res"].repulsion is None and only_r["res"].projection is None
    assert torch.equal(only_p["proj"], both["proj"]) and torch.equal(only_p["gproj"], both["gproj"])
    assert torch.equal(only_r["rep"], both["rep"]) and torch.equal(only_r["grep"], both["grep"])
    # without a gradient asked for the values are the same bits
    from iso_points_amd.loss import surface_losses
    plain = surface_losses(pts.to(dev), nrm.to(dev), torch.tensor(lengths, device=dev))
    assert not plain.projection.requires_grad
    assert torch.equal(plain.projection.cpu(), both["proj"]) and torch.equal(plain.repulsion.cpu(), both["rep"])


# ------------------------------------------------------------------------------------------------ the modules
class _Cloud(object):
    """The part of pytorch3d's Pointclouds the losses use."""

    def __init__(self, pts, nrm, lengths):
        self.pts, self.nrm, self.lengths, self.updated = pts, nrm, lengths, None

    def points_padded(self):
        return self.pts

    def normals_padded(self):
        return self.nrm

    def num_points_per_cloud(self):
        return self.lengths

    def update_normals_(self, packed):
        self.updated = packed


def test_stale_tree_keeps_the_distances_and_positions_it_was_built_with(dev):
    from iso_points_amd.loss import ProjectionLoss, RepulsionLoss
    pts, nrm = _cloud(400, 32)
    g = torch.Generator().manual_seed(5)
    moved = pts + 0.004 * torch.randn(pts.shape, generator=g)
    for cls, name in ((ProjectionLoss, "proj"), (RepulsionLoss, "rep")):
        mod = cls(reduction="none")
        mod((pts[None].to(dev), nrm[None].to(dev)))
        tree = mod.knn_tree
        assert tree is not None and tree.idx.shape == (1, 400, 32)
        p = moved[None].to(dev).requires_grad_(True)
        loss = mod((p, nrm[None].to(dev)), rebuild_knn=False)
        assert mod.knn_tree.idx.data_ptr() == tree.idx.data_ptr() and mod.knn_tree.points.data_ptr() == tree.points.data_ptr()
        grad, = torch.autograd.grad(loss.sum(), p)
        idx, dists = tree.idx[0].cpu(), tree.dists[0].cpu()
        ref = O.sweeps(moved, nrm, idx, dists, dtype=torch.float64, nbr_points=pts)
        f32 = O.sweeps(moved, nrm, idx, dists, dtype=torch.float32, nbr_points=pts)
        assert ref["sum_W"].min().item() >= 1e-12 and (ref["margin"] > 1e-5).all()
        for key, val in ((name, loss), ("g" + name, grad[0])):
            A, err32 = O.tolerance(f32[key], ref[key])
            err = (val.detach().cpu().double() - ref[key].detach()).abs().max().item()
            print("stale tree, %s: oracle float32 error %.3g -> A %.3g; kernel error %.3g" % (key, err32, A, err))
            assert err <= A
        # and it is not what a fresh search gives
        fresh = mod((p, nrm[None].to(dev)), rebuild_knn=True)
        assert not torch.equal(fresh, loss)
        assert mod.knn_tree.idx.data_ptr() != tree.idx.data_ptr()
    assert RepulsionLoss._rebuild_default and not ProjectionLoss._rebuild_default


def test_reductions_and_keyword_overrides(dev):
    from iso_points_amd.loss import ProjectionLoss, RepulsionLoss, surface_losses
    pts, nrm = _cloud(400, 32)
    cloud = (pts[None].to(dev), nrm[None].to(dev))
    for cls, field in ((ProjectionLoss, "projection"), (RepulsionLoss, "repulsion")):
        want = getattr(surface_losses(*cloud), field)
        assert torch.equal(cls(reduction="none")(cloud), want)
        assert torch.equal(cls(reduction="sum")(cloud), want.sum())
        assert torch.equal(cls()(cloud), want.mean())
        mod = cls(knn_k=17)
        assert torch.equal(mod(cloud, reduction="sum"), getattr(surface_losses(*cloud, knn_k=17), field).sum())
        assert mod.reduction == "mean"
        other = getattr(surface_losses(*cloud, knn_k=17, filter_scale=1.5, sharpness_sigma=0.5), field)
        assert not torch.equal(other.mean(), mod(cloud))
        assert torch.equal(mod(cloud, filter_scale=1.5, sharpness_sigma=0.5, rebuild_knn=True), other.mean())
        assert (mod.filter_scale, mod.sharpness_sigma) == (1.5, 0.5)            # kept, as the reference's compute() keeps them
        given = surface_losses(*cloud, knn_k=9).knn
        got = mod(cloud, knn_tree=given, rebuild_knn=False, reduction="none")
        assert mod.knn_tree.idx.shape[2] == 8
        assert torch.equal(got, getattr(surface_losses(*cloud, knn_k=9, filter_scale=1.5, sharpness_sigma=0.5), field))
        with pytest.raises(ValueError):
            mod(cloud, reduction="median")


def test_update_normals_receives_the_packed_mollified_normals(dev):
    from iso_points_amd.loss import ProjectionLoss, surface_losses
    lengths = (400, 64)
    pts, nrm = _padded(lengths, (32, 33))
    lens = torch.tensor(lengths, device=dev)
    cloud = _Cloud(pts.to(dev), nrm.to(dev), lens)
    before = cloud.nrm.clone()
    loss = ProjectionLoss(reduction="none")(cloud)
    want = surface_losses(cloud.pts, cloud.nrm, lens)
    assert cloud.updated.shape == (464, 3)
    assert torch.equal(cloud.updated, torch.cat([want.normals[0, :400], want.normals[1, :64]]))
    assert torch.equal(loss, want.projection)
    assert torch.equal(cloud.nrm.isnan(), before.isnan()) and torch.equal(cloud.nrm[0], before[0])      # tensors untouched
