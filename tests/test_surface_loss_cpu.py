"""The oracle of the point regularisers checked against itself (tests/surface_loss_oracle.py), and the argument checks of
iso_points_amd.loss.surface_losses / ProjectionLoss / RepulsionLoss that need no GPU."""
import pytest
import torch

import surface_loss_oracle as O


def _oracle_inputs(P, K, seed):
    pts, nrm = O.cloud(P, seed)
    _, idx = O.knn_others(pts, K)
    return pts, nrm, idx, O.dists_f32(pts, idx)


def test_closed_form_gradients_equal_autograd_in_float64():
    """The two per-row gradient vectors the kernel writes are the derivatives of the two losses with the weights, the
    normals and the neighbour positions held constant: torch autograd on the oracle's own ops agrees to rounding."""
    pts, nrm, idx, dists = _oracle_inputs(400, 32, seed=3)
    p = pts.double().requires_grad_(True)
    out = O.sweeps(p, nrm, idx, dists, nbr_points=pts.double())
    for loss, closed in (("proj", "gproj"), ("rep", "grep")):
        auto, = torch.autograd.grad(out[loss].sum(), p, retain_graph=True)
        err = (auto - out[closed]).abs().max().item()
        top = out[closed].abs().max().item()
        print("%s: closed form against autograd: worst |d| %.3g at a largest entry of %.3g" % (loss, err, top))
        assert err <= 1e-13 * max(top, 1.0)
    assert out["sum_W"].min().item() >= 1e-12


def test_lifted_lattice_point_projects_to_its_height():
    """A planar lattice, every normal the plane's, one point lifted by h: every s_ik of that row is -h, so D = -h, the
    projection loss is h^2 (13 roundings of 2^-24 on the way: 32 products, two sums of 32, a quotient, a square: within
    2e-6 relative) and the mollified normal stays the plane's.  Spacing and height are powers of two: exact inputs."""
    n, a, h = 9, 1.0 / 16, 1.0 / 64
    lifted = (n // 2) * n + n // 2
    pts, nrm = O.lattice(n, a, lifted, h)
    _, idx = O.knn_others(pts, 32)
    for dtype in (torch.float64, torch.float32):
        out = O.sweeps(pts, nrm, idx, O.dists_f32(pts, idx), dtype=dtype)
        assert abs(out["proj"][lifted].item() - h * h) <= 2e-6 * h * h
        O.assert_plane_normal(out["n2"][lifted])
        assert out["sum_w"][lifted].item() > 0


def test_oracle_others_is_the_sorted_brute_force_without_the_diagonal():
    pts, _ = O.cloud(300, seed=5)
    K = 32
    dists, idx = O.knn_others(pts, K)
    d2 = O.pair_d2(pts)
    order = torch.argsort(d2, dim=1, stable=True)
    rows = torch.arange(300)[:, None]
    keep = order != rows                                   # drop the point itself wherever the sort has put it
    want = order[keep].reshape(300, 299)[:, :K]
    assert torch.equal(idx, want)
    assert torch.equal(dists, d2[rows, want])
    assert (dists[:, 1:] >= dists[:, :-1]).all() and (dists > 0).all()
    assert not (idx == rows).any()


# ------------------------------------------------------------------------------------------------ argument checks
def _cpu_cloud(P=40):
    pts, nrm = O.cloud(P, seed=1)
    return pts[None], nrm[None]


@pytest.mark.parametrize("knn_k", [1, 34, 0, -3])
def test_knn_k_outside_the_range_is_refused(knn_k):
    from iso_points_amd.loss import surface_losses
    pts, nrm = _cpu_cloud()
    with pytest.raises(ValueError, match="knn_k"):
        surface_losses(pts, nrm, knn_k=knn_k)


def test_a_cloud_shorter_than_knn_k_is_refused():
    from iso_points_amd.loss import surface_losses
    pts, nrm = _cpu_cloud(40)
    with pytest.raises(ValueError, match="at least knn_k"):
        surface_losses(pts, nrm, torch.tensor([32]))                       # knn_k = 33 needs 33 points
    two = torch.cat([pts, pts]), torch.cat([nrm, nrm])
    with pytest.raises(ValueError, match="at least knn_k"):
        surface_losses(two[0], two[1], torch.tensor([40, 8]), knn_k=9)
    with pytest.raises(ValueError, match="lengths"):
        surface_losses(pts, nrm, torch.tensor([41]))


def test_a_normals_shape_mismatch_is_refused():
    from iso_points_amd.loss import surface_losses
    pts, nrm = _cpu_cloud()
    with pytest.raises(ValueError, match="normals"):
        surface_losses(pts, nrm[:, :-1])
    with pytest.raises(ValueError, match="normals"):
        surface_losses(pts, None)
    with pytest.raises(ValueError):
        surface_losses(pts, nrm, projection=False, repulsion=False)


def test_points_filters_are_not_implemented():
    from iso_points_amd.loss import ProjectionLoss, RepulsionLoss
    pts, nrm = _cpu_cloud()
    for mod in (ProjectionLoss(), RepulsionLoss()):
        with pytest.raises(NotImplementedError, match="losses.py:214"):
            mod((pts, nrm), points_filters=object())
    with pytest.raises(ValueError):
        ProjectionLoss(reduction="median")


def test_cpu_tensors_are_refused():
    from iso_points_amd.loss import ProjectionLoss, surface_losses
    from iso_points_amd.point_processing import knn_others
    pts, nrm = _cpu_cloud()
    with pytest.raises(RuntimeError, match="GPU"):
        surface_losses(pts, nrm, knn_k=9)
    with pytest.raises(RuntimeError, match="GPU"):
        ProjectionLoss(knn_k=9)((pts, nrm))
    with pytest.raises(RuntimeError, match="GPU"):
        knn_others(pts, K=8)
    with pytest.raises(ValueError):
        knn_others(pts, K=33)


def test_module_defaults_follow_the_reference():
    from iso_points_amd.loss import ProjectionLoss, RepulsionLoss
    p, r = ProjectionLoss(), RepulsionLoss()
    for m in (p, r):
        assert (m.reduction, m.knn_k, m.filter_scale, m.sharpness_sigma, m.knn_tree) == ("mean", 33, 2.0, 0.75, None)
    assert p._rebuild_default is False and r._rebuild_default is True
