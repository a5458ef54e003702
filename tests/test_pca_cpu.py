"""Local frames of a K-neighbourhood (DSS/utils/mathHelper.py:43-119) on the CPU.

  * A float64 numpy restatement of the contract of iso_pca_frames -- eigh of the centred neighbourhood covariance, ascending,
    clamped at 0, and the reference's sign rule tested against the globally centred point (d_j = x_j - (p_i - mu_b)) --
    reproduces every tests/golden/pca_*.npz (the reference's own function, tests/golden/make_golden_pca.py).  The GPU tests
    use the same restatement and the same judge on clouds too large for fixtures.
  * The Python entry points refuse CPU tensors, neighborhood_size >= num_points and neighborhood_size > 32 before any GPU
    call (these run on a machine without one)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
PCA_FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "pca_*.npz")))


def load(name):
    d = np.load(os.path.join(GOLDEN, name))
    return {k: np.asarray(d[k]) for k in d.files}


def restate_rows(cloud, nbr, rows, mu, disambiguate):
    """float64 contract for query rows `rows` (R,) of one cloud (L,3) with neighbour indices nbr (R,K) and cloud mean mu.
    Returns curvature (R,3), frames (R,3,3) and, per sign-ruled column (0 and 2), n_pos (R,) and the smallest
    |<v, d_j>| / |d_j| (R,) -- the two quantities the sign exemptions are judged on."""
    cloud = np.asarray(cloud, dtype=np.float64)
    X = cloud[nbr]                                                       # (R,K,3)
    K = nbr.shape[1]
    D = X - X.mean(axis=1, keepdims=True)
    C = np.einsum("rki,rkj->rij", D, D) / K
    w, V = np.linalg.eigh(C)                                             # ascending; V[..., c] = eigenvector c
    w = np.maximum(w, 0.0)
    aux = {}
    if disambiguate:
        d = X - (cloud[rows] - mu)[:, None, :]
        dn = np.linalg.norm(d, axis=-1)
        for col in (0, 2):
            proj = np.einsum("rkc,rc->rk", d, V[:, :, col])
            n_pos = (proj > 0).sum(axis=1)
            V[:, :, col] *= np.where(n_pos < 0.5 * K, -1.0, 1.0)[:, None]
            aux[col] = (n_pos, (np.abs(proj) / np.maximum(dn, 1e-300)).min(axis=1))
        V[:, :, 1] = np.cross(V[:, :, 0], V[:, :, 2])
    return w, V, aux


def restate(points, num_points, idx, disambiguate):
    """restate_rows over every valid row of a padded batch: lists per cloud."""
    points, idx = np.asarray(points, dtype=np.float64), np.asarray(idx)
    out = []
    for b, L in enumerate(int(x) for x in np.asarray(num_points)):
        rows = np.arange(L)
        out.append(restate_rows(points[b, :L], idx[b, :L], rows, points[b, :L].mean(axis=0), disambiguate))
    return out


def judge(curv, frames, ref_curv, ref_frames, K, aux=None, what=""):
    """The parity criteria of the local-frame estimator, on the valid rows of one cloud (numpy, any float type):
      eigenvalues within 2e-5 lambda_max + 1e-12 of the reference's;
      each eigenvector i: |sin angle(v_i, v_i_ref)| <= 1e-4 where gap_i >= 1e-2 lambda_max (gap_i = distance to the nearest
      other reference eigenvalue);
      frames orthonormal within 1e-5 everywhere;
      with `aux` (disambiguation): columns 0 and 2 point the reference's way on every such point, except where some
      |<v, d_j>| <= 1e-6 |d_j| or n_pos lies within one of K/2 (exempt: fewer than 0.5 % of the rows).  Mismatches at
      n_pos == K/2 exactly are counted apart as undetermined: there the rule leaves the eigensolver's own sign.
    Returns (exempt sign mismatches, undetermined sign mismatches, number of rows)."""
    curv, frames = np.asarray(curv, np.float64), np.asarray(frames, np.float64)
    ref_curv, ref_frames = np.asarray(ref_curv, np.float64), np.asarray(ref_frames, np.float64)
    R = curv.shape[0]
    lmax = ref_curv.max(axis=1)
    err = np.abs(curv - ref_curv).max(axis=1)
    bad = err > 2e-5 * lmax + 1e-12
    assert not bad.any(), "%s: %d of %d eigenvalue triples off (worst %g of lambda_max)" % (
        what, bad.sum(), R, (err / np.maximum(lmax, 1e-300)).max())
    gtg = np.einsum("rki,rkj->rij", frames, frames)
    orth = np.abs(gtg - np.eye(3)).max(axis=(1, 2))
    assert np.isfinite(frames).all() and orth.max() <= 1e-5, "%s: frames not orthonormal (worst %g)" % (what, orth.max())
    exempt = undetermined = 0
    for i in range(3):
        others = [j for j in range(3) if j != i]
        gap = np.minimum(np.abs(ref_curv[:, i] - ref_curv[:, others[0]]), np.abs(ref_curv[:, i] - ref_curv[:, others[1]]))
        sel = (gap >= 1e-2 * lmax) & (lmax > 0)
        v, vr = frames[:, :, i], ref_frames[:, :, i]
        sin = np.linalg.norm(np.cross(v, vr), axis=1) / np.maximum(np.linalg.norm(v, axis=1) * np.linalg.norm(vr, axis=1), 1e-300)
        bad = sel & (sin > 1e-4)
        assert not bad.any(), "%s: eigenvector %d: %d of %d well-separated points beyond 1e-4 (worst sin %g)" % (
            what, i, bad.sum(), sel.sum(), sin[sel].max())
        if aux is not None and i in aux:
            n_pos, margin = aux[i]
            flipped = sel & ((v * vr).sum(axis=1) < 0)
            # n_pos == K/2 exactly: neither v nor -v has fewer than K/2 positive projections, so the rule keeps whatever
            # sign the eigensolver produced -- the reference's answer there is its SVD's convention, not the rule's
            tie = 2 * n_pos == K
            excused = (np.abs(n_pos - 0.5 * K) <= 1) | (margin <= 1e-6)
            assert not (flipped & ~excused).any(), "%s: column %d: %d points with the other sign and no excuse" % (
                what, i, (flipped & ~excused).sum())
            exempt += int((flipped & ~tie).sum())
            undetermined += int((flipped & tie).sum())
    assert exempt < 0.005 * R, "%s: %d exempt sign mismatches of %d points" % (what, exempt, R)
    return exempt, undetermined, R


@pytest.mark.parametrize("name", PCA_FILES)
def test_restatement_reproduces_the_reference_fixture(name):
    g = load(name)
    K = int(g["K"])
    assert g["idx"].shape[-1] == K
    for tag, dis in (("dis", True), ("raw", False)):
        for b, (w, V, aux) in enumerate(restate(g["points"], g["num_points"], g["idx"], dis)):
            L = int(g["num_points"][b])
            judge(w, V, g["curvature_" + tag][b, :L], g["frames_" + tag][b, :L], K, aux if dis else None,
                  "%s cloud %d %s" % (name, b, tag))
            # float64 against float64: the eigenvalues agree to rounding
            assert np.abs(w - g["curvature_" + tag][b, :L]).max() <= 1e-12 * g["curvature_" + tag][b, :L].max()


def test_fixtures_cover_the_cases_the_issue_names():
    assert {"pca_sphere_K8.npz", "pca_sphere_K16.npz", "pca_cube_K12.npz", "pca_ragged_K16.npz",
            "pca_translated_K16.npz"} <= set(PCA_FILES)
    g = load("pca_translated_K16.npz")
    # the centred-versus-uncentred composition of the sign rule matters here: the rule applied to p_i instead of
    # p_i - mu flips a large share of the normals
    w, V, aux = restate(g["points"], g["num_points"], g["idx"], True)[0]
    L = int(g["num_points"][0])
    pts, idx = g["points"][0, :L].astype(np.float64), g["idx"][0, :L]
    d = pts[idx] - pts[:, None, :]
    n_pos = (np.einsum("rkc,rc->rk", d, V[:, :, 0]) > 0).sum(axis=1)
    assert (n_pos < 8).mean() > 0.05
    for name in PCA_FILES:
        g = load(name)
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20
        for k in (16, 31):
            ratio, mask = g["outlier_ratio_K%d" % k], g["outlier_mask_K%d" % k]
            assert mask.any() and not mask.all()
            inside = np.arange(mask.shape[1])[None, :] < g["num_points"][:, None]
            assert ((ratio < g["tolerance"]) & inside == mask).all()


def _cloud(P=200):
    g = torch.Generator().manual_seed(0)
    return torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1)


def test_entry_points_refuse_cpu_tensors():
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals
    from iso_points_amd.point_processing import remove_outliers
    x = _cloud()
    for fn in (lambda: estimate_pointcloud_local_coord_frames(x, neighborhood_size=8),
               lambda: estimate_pointcloud_normals(x, neighborhood_size=8),
               lambda: remove_outliers(x, neighborhood_size=8)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()


def test_entry_points_refuse_neighbourhoods_they_cannot_serve():
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames, estimate_pointcloud_normals
    from iso_points_amd.point_processing import remove_outliers
    x = _cloud(20)
    for K in (20, 21):                                                   # num_points <= neighborhood_size (:66)
        with pytest.raises(ValueError):
            estimate_pointcloud_local_coord_frames(x, neighborhood_size=K)
        with pytest.raises(ValueError):
            remove_outliers(x, neighborhood_size=K)
    with pytest.raises(ValueError):
        estimate_pointcloud_normals(x)                                   # the default of 50
    big = _cloud(200)
    for fn in (lambda: estimate_pointcloud_local_coord_frames(big, neighborhood_size=33),
               lambda: estimate_pointcloud_normals(big)):
        with pytest.raises(NotImplementedError, match="32"):
            fn()
    # ragged lengths: the shortest cloud decides
    pad = torch.cat([big, big], 0)

    class PC(object):
        def points_padded(self):
            return pad

        def num_points_per_cloud(self):
            return torch.tensor([200, 12])
    with pytest.raises(ValueError):
        estimate_pointcloud_local_coord_frames(PC(), neighborhood_size=12)
    with pytest.raises(ValueError):
        estimate_pointcloud_local_coord_frames(torch.rand(1, 50, 2), neighborhood_size=8)


def test_no_backward_and_no_silent_detach():
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames
    x = _cloud().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="backward"):
        estimate_pointcloud_local_coord_frames(x, neighborhood_size=8)
    with torch.no_grad():                                   # the trainer's call: past the grad check, on to the CPU refusal
        with pytest.raises(RuntimeError, match="GPU"):
            estimate_pointcloud_local_coord_frames(x, neighborhood_size=8)
