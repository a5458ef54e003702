"""Golden vectors for the two non-default splat variances (DSS/core/rasterizer.py:257-342, 417-424): the reference's own
SurfaceSplatting._get_per_point_info is imported from the checkout AT GENERATION TIME and run with Vrk_isotropic=False
(anisotropic) and with Vrk_invariant=True (invariant); only inputs and results are stored (vrk_*.npz).

Stand-ins, as in make_golden_splat.py (cameras, point-cloud container) and make_golden_pca.py (kNN = the oracle's brute
force, batch_svd = torch.linalg.svd): the rasterizer module's estimate_pointcloud_local_coord_frames is set to the
reference's own mathHelper function loaded that way.  Every scene is run twice: in float64 on the float32-rounded inputs
(the truth) and in float32 (the yardstick a float32 implementation is held against).  FRNN distances are the float32
values of the FRNN contract in both runs (they are data of the neighbour search, bit-exact on the GPU); the float64 run
takes their mean in double.

usage:  python tests/golden/make_golden_vrk.py        (writes tests/golden/vrk_*.npz)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GAP = 0.02          # (l1 - l0) / l2 below which "which direction is the normal" is ill-posed
GAP_CAP = 0.01      # at most this share of a scene's rows may be that ill-posed


class _Clouds(object):
    """The accessors _get_per_point_info uses, in the dtype of the lists."""

    def __init__(self, pts_list, nrm_list):
        self.p, self.n = pts_list, nrm_list
        self.num = torch.tensor([len(x) for x in pts_list])

    def __len__(self):
        return len(self.p)

    def points_packed(self):
        return torch.cat(self.p, 0)

    def normals_packed(self):
        return torch.cat(self.n, 0)

    def num_points_per_cloud(self):
        return self.num

    def cloud_to_packed_first_idx(self):
        return torch.cumsum(self.num, 0) - self.num

    def packed_to_cloud_idx(self):
        return torch.repeat_interleave(torch.arange(len(self.p)), self.num)

    def points_padded(self):
        out = torch.zeros(len(self.p), int(self.num.max()), 3, dtype=self.p[0].dtype)
        for i, x in enumerate(self.p):
            out[i, : len(x)] = x
        return out


class _Transform(object):
    def __init__(self, m):
        self.m = m

    def get_matrix(self):
        return self.m


class _Cameras(object):
    """The full world -> NDC matrices are inputs (float32 products, as a caller hands them to the GPU), not recomputed."""

    def __init__(self, views, projs):
        self.views, self.projs = views, projs
        self.R = views[:, :3, :3]

    def get_full_projection_transform(self, **kw):
        return _Transform(self.projs)


def cube_scene(P, n_views, S, seed, jitter):
    """Points on the surface of [-0.3, 0.3]^3 (faces, edges, corners) with the face normals, filtered per view the way
    splat_util.sphere_scene filters its sphere.  The size puts the mean bandwidth of the largest view cloud between the
    invariant mode's clamps (5e-5, 1e-3), so that the mean itself is pinned and not only the clamp."""
    from oracle import splat_oracle as SO
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(P, 3, generator=g) * 2 - 1
    face = torch.randint(0, 6, (P,), generator=g)
    ax, sgn = face % 3, (face // 3).float() * 2 - 1
    u[torch.arange(P), ax] = sgn
    nrm = torch.zeros(P, 3)
    nrm[torch.arange(P), ax] = sgn
    pts = 0.3 * (u + jitter * (torch.rand(P, 3, generator=g) - 0.5))
    Vs = [SO.look_at_view(3.0, 25.0, 30.0 + 360.0 * i / n_views) for i in range(n_views)]
    keep = [SO.filter_renderable(pts, nrm, V) for V in Vs]
    num = torch.tensor([int(m.sum()) for m in keep])
    return {"points": torch.cat([pts[m] for m in keep]), "normals": torch.cat([nrm[m] for m in keep]), "num": num,
            "views": torch.stack(Vs), "proj": SO.perspective(30.0), "S": S}


def run_reference(R, MH, sc, mode, dtype, frnn_radius):
    """_get_per_point_info of the reference in `mode` and `dtype`; also the per-view kNN index and the per-row curvature
    (anisotropic) or the per-row h (invariant) it used, each recorded from the reference's own calls."""
    import frnn as frnn_stub
    from oracle import iso_oracle as O
    num = sc["num"].tolist()
    clouds = _Clouds([x.to(dtype) for x in torch.split(sc["points"], num)],
                     [x.to(dtype) for x in torch.split(sc["normals"], num)])
    cams = _Cameras(sc["views"].to(dtype), torch.stack([v @ sc["proj"] for v in sc["views"]]).to(dtype))
    rs = R.PointsRasterizationSettings(image_size=sc["S"], points_per_pixel=8, cutoff_threshold=1.0, antialiasing_sigma=1.0,
                                       Vrk_isotropic=(mode != "aniso"), Vrk_invariant=(mode == "invariant"))
    obj = object.__new__(R.SurfaceSplatting)
    obj.raster_settings, obj.cameras, obj.frnn_radius, obj._Vrk_h = rs, cams, frnn_radius, None
    seen = {}

    def frames(pc, neighborhood_size=50, disambiguate_directions=True, **kw):
        curv, fr, knn = MH.estimate_pointcloud_local_coord_frames(pc, neighborhood_size=neighborhood_size,
                                                                  disambiguate_directions=disambiguate_directions,
                                                                  return_knn_result=True)
        seen["curvature"], seen["idx"] = curv, knn.idx
        return curv, fr

    def frnn_grid_points(p1, p2, l1=None, l2=None, K=-1, r=-1, **kw):
        d, i, nn, grid = O.frnn_grid_points(p1, p2, l1, l2, K=K, r=r)
        seen["dists"] = d
        return d.to(dtype), i, nn, grid

    gather = getattr(R.gather_batch_to_packed, "_vrk_wrapped", R.gather_batch_to_packed)

    def gather_batch_to_packed(data, batch_idx):
        if data.dim() == 3 and tuple(data.shape[1:]) == (1, 1):          # h_k (N,1,1); W and M44 slices are (N,3,4) / (N,4,k)
            seen["h_k"] = data.detach().clone()
        return gather(data, batch_idx)

    gather_batch_to_packed._vrk_wrapped = gather
    R.gather_batch_to_packed = gather_batch_to_packed
    R.estimate_pointcloud_local_coord_frames = frames
    frnn_stub.frnn_grid_points = frnn_grid_points
    torch.manual_seed(0)   # the invariant mode's tangent frame uses torch.rand_like (rasterizer.py:338-339)
    info = R.SurfaceSplatting._get_per_point_info(obj, clouds, cameras=cams, raster_settings=rs)
    out = {k: info[k] for k in ("radii", "ellipse_params", "cutoff_threshold", "scaler")}
    if mode == "aniso":
        out["curvature"] = torch.cat([seen["curvature"][b, :n] for b, n in enumerate(num)])
        out["idx"] = seen["idx"]
    else:
        # the cloud's h is the reference's own tensor: the argument of the gather_batch_to_packed call that spreads it over
        # the rows (rasterizer.py:327-328), recorded below
        h = seen["h_k"].reshape(-1)
        out["h"] = torch.cat([h[b].expand(n) for b, n in enumerate(num)])
        out["dists"] = seen["dists"]
    return out


def gen_vrk():
    from make_golden import install_shims, npz
    from make_golden_pca import load_mh
    from make_golden_splat import load_reference_rasterizer
    install_shims()
    MH = load_mh()
    import DSS
    import make_golden
    DSS._C = sys.modules["DSS._C"] = make_golden._Stub("DSS._C")      # the compiled extension: imported, never called here
    R = load_reference_rasterizer()
    from splat_util import sphere_scene
    sph = sphere_scene(3000, n_views=3, S=64, seed=21)
    sph = {k: sph[k] for k in ("points", "normals", "num", "views", "proj", "S")}
    scenes = (("sphere", sph, 0.2), ("cube", cube_scene(3600, n_views=2, S=64, seed=5, jitter=0.01), 0.2))
    for name, sc, radius in scenes:
        arrays = {"points": sc["points"], "normals": sc["normals"], "num": sc["num"], "views": sc["views"],
                  "proj": sc["proj"], "projs": torch.stack([v @ sc["proj"] for v in sc["views"]]), "image_size": sc["S"], "cutoff": 1.0, "sigma": 1.0, "frnn_radius": radius}
        for mode in ("aniso", "invariant"):
            for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
                out = run_reference(R, MH, sc, mode, dtype, radius)
                for k, v in out.items():
                    if k == "idx":
                        if "knn_idx" in arrays:
                            assert torch.equal(arrays["knn_idx"].long(), v), "kNN index differs between precisions"
                        arrays["knn_idx"] = v.short()          # int16 on disk: a view cloud here holds < 2^15 points
                    elif k == "dists":
                        arrays["frnn_dists"] = v[:, :, :7]
                    else:
                        arrays["%s_%s_%s" % (mode, k, tag)] = v
        l = arrays["aniso_curvature_f64"]
        gap = (l[:, 1] - l[:, 0]) / l[:, 2]
        share = (gap < GAP).double().mean().item()
        print("%s: view clouds %s; rows with (l1 - l0) / l2 < %.2f: %.4f %% (cap %.1f %%); invariant h per view %s"
              % (name, sc["num"].tolist(), GAP, 100 * share, 100 * GAP_CAP,
                 sorted(set(arrays["invariant_h_f64"].tolist()))))
        assert share < GAP_CAP, "lower the jitter, not the cap"
        del arrays["frnn_dists"]                 # (kept out: the test queries FRNN itself; the index pins the anisotropic search)
        npz("vrk_%s.npz" % name, **arrays)


if __name__ == "__main__":
    gen_vrk()
