"""Local frames of a K-neighbourhood (iso_pca_frames, DSS/utils/mathHelper.py:43-119) on the GPU.

  * parity with the reference's own function (tests/golden/pca_*.npz), with and without the sign rule, judged by
    tests/test_pca_cpu.py::judge;
  * the same criteria against the float64 restatement on a 100 k-point sphere and on a cloud with exact duplicates and a
    collinear run (finite, orthonormal, lambda >= 0 everywhere);
  * remove_outliers against the fixtures' masks, order and lengths;
  * a 1 M-point repeat run at K = 16: bit-identical, no NaN, a 10 k-row sample against float64;
  * padded rows are zero; return_knn_result returns knn_points' own tuple; the normals are column 0 bit for bit."""
import numpy as np
import pytest
import torch

from test_pca_cpu import PCA_FILES, judge, load, restate, restate_rows

pytestmark = pytest.mark.gpu


def _run(g, dev, dis, return_knn=False):
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames

    class PC(object):
        def points_padded(self):
            return torch.from_numpy(g["points"]).to(dev)

        def num_points_per_cloud(self):
            return torch.from_numpy(g["num_points"]).to(dev)
    return estimate_pointcloud_local_coord_frames(PC(), neighborhood_size=int(g["K"]), disambiguate_directions=dis,
                                                  return_knn_result=return_knn)


@pytest.mark.parametrize("name", PCA_FILES)
def test_frames_match_the_reference_fixture(dev, name):
    from iso_points_amd.math_helper import estimate_pointcloud_normals
    g = load(name)
    K = int(g["K"])
    for tag, dis in (("dis", True), ("raw", False)):
        curv, frames, knn = _run(g, dev, dis, return_knn=True)
        torch.cuda.synchronize()
        c, f = curv.cpu().numpy(), frames.cpu().numpy()
        assert (c >= 0).all()
        ours = restate(g["points"], g["num_points"], knn.idx.cpu().numpy(), dis)
        for b in range(g["points"].shape[0]):
            L = int(g["num_points"][b])
            assert (knn.idx[b, :L].cpu().numpy() == g["idx"][b, :L]).all(), "the exact kNN differs from the fixture's"
            ex, und, R = judge(c[b, :L], f[b, :L], g["curvature_" + tag][b, :L], g["frames_" + tag][b, :L], K,
                               ours[b][2] if dis else None, "%s cloud %d %s" % (name, b, tag))
            print("%s cloud %d %s: %d exempt, %d undetermined sign mismatches of %d" % (name, b, tag, ex, und, R))
            # padded rows are zero
            assert (c[b, L:] == 0).all() and (f[b, L:] == 0).all()
        if dis:
            # estimate_pointcloud_normals is column 0, bit for bit
            nrm = estimate_pointcloud_normals(_PC(g, dev), neighborhood_size=K)
            assert torch.equal(nrm, frames[:, :, :, 0])


class _PC(object):
    def __init__(self, g, dev):
        self.g, self.dev = g, dev

    def points_padded(self):
        return torch.from_numpy(self.g["points"]).to(self.dev)

    def num_points_per_cloud(self):
        return torch.from_numpy(self.g["num_points"]).to(self.dev)


def test_return_knn_result_is_knn_points_own_tuple(dev):
    from iso_points_amd.point_processing import knn_points
    g = load("pca_ragged_K16.npz")
    _, _, knn = _run(g, dev, True, return_knn=True)
    pts, num = torch.from_numpy(g["points"]).to(dev), torch.from_numpy(g["num_points"]).to(dev)
    want = knn_points(pts, pts, num, num, K=16, return_nn=True)
    assert type(knn).__name__ == "KNN" and knn._fields == want._fields
    for a, b in zip(knn, want):
        assert torch.equal(a, b)


def _against_float64(pts, K, dev, what, degenerate=False):
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames
    x = torch.from_numpy(pts).to(dev)
    n = torch.tensor([pts.shape[1]], device=dev)
    for dis in (True, False):
        curv, frames, knn = estimate_pointcloud_local_coord_frames(_Raw(x, n), neighborhood_size=K,
                                                                   disambiguate_directions=dis, return_knn_result=True)
        c, f = curv[0].cpu().numpy(), frames[0].cpu().numpy()
        assert np.isfinite(c).all() and np.isfinite(f).all() and (c >= 0).all(), what
        w, V, aux = restate(pts, np.array([pts.shape[1]]), knn.idx.cpu().numpy(), dis)[0]
        if degenerate:
            # the degenerate rows (lambda_max = 0: all neighbours one point) are judged on orthonormality alone
            judge(c, f, w, V, K, aux if dis else None, what)
        else:
            ex, und, R = judge(c, f, w, V, K, aux if dis else None, what)
            print("%s dis=%s: %d exempt, %d undetermined of %d" % (what, dis, ex, und, R))


class _Raw(object):
    def __init__(self, p, n):
        self.p, self.n = p, n

    def points_padded(self):
        return self.p

    def num_points_per_cloud(self):
        return self.n


def test_frames_on_a_100k_sphere_match_float64(dev):
    g = torch.Generator().manual_seed(5)
    pts = torch.nn.functional.normalize(torch.randn(1, 100_000, 3, generator=g), dim=-1).numpy()
    _against_float64(pts, 16, dev, "100 k sphere K=16")


def test_frames_with_duplicates_and_a_collinear_run_are_finite(dev):
    g = torch.Generator().manual_seed(6)
    sph = torch.nn.functional.normalize(torch.randn(3000, 3, generator=g), dim=-1)
    dup = sph[:1].repeat(40, 1) * 1.5                                   # 40 copies of one point: C = 0
    line = torch.stack([torch.linspace(-2, -1.5, 40), torch.zeros(40) + 0.25, torch.zeros(40) - 0.5], dim=1)   # rank 1
    pts = torch.cat([sph, dup, line], 0)[None].contiguous().numpy()
    _against_float64(pts, 16, dev, "duplicates + collinear K=16", degenerate=True)
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames
    curv, _ = estimate_pointcloud_local_coord_frames(torch.from_numpy(pts).to(dev), neighborhood_size=16)
    assert (curv[0, 3000:3040] == 0).all(), "K exact duplicates: the covariance is exactly zero"
    # remove_outliers on it: the duplicates' ratio is 0 / 0 = NaN and they are dropped, as in the reference
    from iso_points_amd.point_processing import remove_outliers
    out, n = remove_outliers(torch.from_numpy(pts).to(dev), neighborhood_size=16)
    kept = out[0, : int(n[0])].cpu()
    assert not (kept == torch.from_numpy(pts[0, 3000])).all(dim=1).any()


@pytest.mark.parametrize("name", PCA_FILES)
def test_remove_outliers_matches_the_fixture_mask(dev, name):
    from iso_points_amd.point_processing import remove_outliers
    g = load(name)
    pts, num = g["points"], g["num_points"]
    for K in (16, 31):
        out, n = remove_outliers(_PC(g, dev), neighborhood_size=K, tolerance=float(g["tolerance"]))
        out, n = out.cpu().numpy(), n.cpu().numpy()
        assert out.shape[1] == n.max()
        mask, ratio = g["outlier_mask_K%d" % K], g["outlier_ratio_K%d" % K]
        for b in range(pts.shape[0]):
            L = int(num[b])
            row_of = {tuple(p): i for i, p in enumerate(pts[b, :L].tolist())}
            sel = np.array([row_of[tuple(p)] for p in out[b, : n[b]].tolist()], dtype=np.int64)
            assert (np.diff(sel) > 0).all(), "compaction must keep the order"
            assert (out[b, n[b]:] == 0).all()
            got = np.zeros(L, dtype=bool)
            got[sel] = True
            near = np.abs(ratio[b, :L] - float(g["tolerance"])) <= 1e-5
            diff = (got != mask[b, :L]) & ~near
            assert not diff.any(), "%s K=%d cloud %d: %d points decided differently" % (name, K, b, diff.sum())
            assert n[b] == got.sum()


def test_frames_repeat_1m_points_k16(dev):
    from iso_points_amd.math_helper import estimate_pointcloud_local_coord_frames
    g = torch.Generator().manual_seed(9)
    P = 1_000_000
    p = torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1)
    p = p + 0.01 * (torch.rand(1, P, 3, generator=g) - 0.5)
    x = p.to(dev)
    c1, f1, knn = estimate_pointcloud_local_coord_frames(x, neighborhood_size=16, return_knn_result=True)
    c2, f2 = estimate_pointcloud_local_coord_frames(x, neighborhood_size=16)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2) and torch.equal(f1, f2), "two runs differ"
    assert not torch.isnan(c1).any() and not torch.isnan(f1).any()
    rows = torch.randperm(P, generator=g)[:10_000].sort().values.numpy()
    cloud = p[0].double().numpy()
    w, V, aux = restate_rows(cloud, knn.idx[0].cpu().numpy()[rows], rows, cloud.mean(axis=0), True)
    ex, und, R = judge(c1[0].cpu().numpy()[rows], f1[0].cpu().numpy()[rows], w, V, 16, aux, "1 M sample")
    print("1 M K=16 sample: %d exempt, %d undetermined of %d" % (ex, und, R))
