"""Float64 restatement of the two non-default splat variances (DSS/core/rasterizer.py:257-342, 417-424, 441-563) and the
judge of the GPU tests, shared by tests/test_vrk_cpu.py and tests/test_vrk_gpu.py.  Fixtures: tests/golden/vrk_*.npz
(the reference's own _get_per_point_info, tests/golden/make_golden_vrk.py)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = ("sphere", "cube")
KEYS = ("radii", "ellipse_params", "cutoff_threshold", "scaler")
GAP = 0.02            # rows whose float64 fixture has (l1 - l0) / l2 below this may be left out of the anisotropic comparison
GAP_CAP = 0.01        # ... and at most this share of a scene's rows


def load(scene):
    d = np.load(os.path.join(GOLDEN, "vrk_%s.npz" % scene))
    return {k: torch.from_numpy(np.asarray(d[k])) if np.asarray(d[k]).ndim else np.asarray(d[k]).item() for k in d.files}


def view_slices(num):
    at = 0
    for n in [int(x) for x in num.tolist()]:
        yield at, n
        at += n


def wjk(points, M44):
    """_compute_WJk for one view (:441-492), float64: (P,3,2)."""
    P = points.shape[0]
    ph = torch.cat([points, torch.ones_like(points[:, :1])], dim=-1)
    t = ph @ M44[:, 3]
    xy = ph @ M44[:, :2]
    t2 = torch.where((t * t).abs() < 1e-17, torch.full_like(t, 1e-17), t * t)
    td = torch.where(t.abs() < 1e-17, torch.full_like(t, 1e-17), t)
    Jk = points.new_zeros(P, 4, 2)
    Jk[:, 0, 0] = 1 / td
    Jk[:, 1, 1] = 1 / td
    Jk[:, 3, 0] = -1 / t2 * xy[:, 0]
    Jk[:, 3, 1] = -1 / t2 * xy[:, 1]
    return M44[:3, :].expand(P, 3, 4) @ Jk


def finish(Mk, c1, c2, S, sigma, cutoff):
    """Ellipse, radii and scaler from Mk (P,2,2) and the two variances (:499-563)."""
    lp = sigma * (2.0 / S) ** 2
    G = Mk.transpose(1, 2) @ torch.diag_embed(torch.stack([c1, c2], -1)) @ Mk + lp * torch.eye(2, dtype=Mk.dtype)
    Ginv = torch.inverse(G)
    a, b, c = Ginv[:, 0, 0], Ginv[:, 0, 1] + Ginv[:, 1, 0], Ginv[:, 1, 1]
    den = 4 * a * c - b * b
    den = torch.where(den.abs() < 1e-17, torch.full_like(den, 1e-17), den)
    eps = lambda x: torch.where(x.abs() < 1e-17, torch.full_like(x, 1e-17), x.abs())       # noqa: E731  (eps_sqrt)
    radii = torch.stack([torch.sqrt(eps(4 * c * cutoff / den)), torch.sqrt(eps(4 * a * cutoff / den))], -1)
    sc = torch.sqrt(eps(torch.det(G) * 4 * np.pi * np.pi))
    sc = torch.det(Mk).abs() / torch.where(sc.abs() < 1e-17, torch.full_like(sc, 1e-17), sc)
    return {"radii": radii, "ellipse_params": torch.stack([a, b, c], -1), "cutoff_threshold": torch.full_like(a, cutoff),
            "scaler": sc}


def restate_aniso(g):
    """Anisotropic mode, float64, from the fixture's inputs and kNN index: (info dict, curvature (P,3))."""
    out, curv = {k: [] for k in KEYS}, []
    pts = g["points"].double()
    for v, (at, n) in enumerate(view_slices(g["num"])):
        cloud = pts[at:at + n]
        X = cloud[g["knn_idx"][v, :n].long()]                                  # (n,8,3)
        D = X - X.mean(dim=1, keepdim=True)
        C = torch.einsum("rki,rkj->rij", D, D) / X.shape[1]
        w, V = torch.linalg.eigh(C)
        w = w.clamp(min=0)
        Sk = V[:, :, 1:].transpose(1, 2)                                       # rows u, v
        M44 = g["projs"][v].double()
        info = finish(Sk @ wjk(cloud, M44), w[:, 1], w[:, 2], g["image_size"], g["sigma"], g["cutoff"])
        for k in KEYS:
            out[k].append(info[k])
        curv.append(w)
    return {k: torch.cat(x) for k, x in out.items()}, torch.cat(curv)


def restate_invariant_h(g, dists=None):
    """One h per view cloud with the reference's padded mean (:322-327), float64 on the float32 FRNN distances.
    dists: (N, >= max num, 7) of the K = 7 self query (the oracle's brute force when None)."""
    num = g["num"]
    if dists is None:
        from oracle import iso_oracle as O
        pmax = int(num.max())
        padded = torch.zeros(len(num), pmax, 3)
        for v, (at, n) in enumerate(view_slices(num)):
            padded[v, :n] = g["points"][at:at + n]
        dists = O.frnn_grid_points(padded, padded, num, num, K=7, r=g["frnn_radius"])[0]
    pmax = int(num.max())
    sq = dists[:, :pmax, 1:].double().clone()
    for v, n in enumerate(num.tolist()):
        sq[v, n:] = -1.0                                                       # FRNN's padding of the rows that do not exist
    sq[num < 7] = 1e-3
    h = (0.5 * sq.max(dim=-1)[0]).mean(dim=1).clamp(5e-5, 1e-3)
    return torch.cat([h[v].expand(n) for v, n in enumerate(num.tolist())])


def restate_invariant(g, h):
    """Invariant mode, float64: isotropic formulas with one h per cloud and any frame orthogonal to the normal."""
    from oracle import splat_oracle as SO
    out = {k: [] for k in KEYS}
    for v, (at, n) in enumerate(view_slices(g["num"])):
        info = SO.per_point_info(g["points"][at:at + n], g["normals"][at:at + n], h[at:at + n],
                                 g["projs"][v], g["image_size"], cutoff=g["cutoff"], sigma=g["sigma"],
                                 dtype=torch.float64)
        for k in KEYS:
            out[k].append(info[k])
    return {k: torch.cat(x) for k, x in out.items()}


def row_err(got, truth):
    """Per row: largest deviation relative to the row's largest component of the truth."""
    t = truth.double().reshape(truth.shape[0], -1)
    x = got.double().reshape(truth.shape[0], -1)
    return ((x - t).abs() / t.abs().amax(-1, keepdim=True)).amax(-1)


def well_posed_rows(g):
    l = g["aniso_curvature_f64"]
    keep = (l[:, 1] - l[:, 0]) / l[:, 2] >= GAP
    assert (~keep).double().mean().item() <= GAP_CAP
    return keep


def judge(name, got, truth, ref32, keep=None):
    """The bar of tests/test_splat_gpu.py::test_setup_matches_oracle: float64 fixture = truth, the reference's float32 run =
    yardstick.  Worst row no further from the truth than 3x the float32 reference's worst + 2e-6, fewer than 1 % of the
    rows beyond 1e-5, median below 1e-6."""
    e_got, e_ref = row_err(got, truth), row_err(ref32, truth)
    if keep is not None:
        e_got, e_ref = e_got[keep], e_ref[keep]
    frac = (e_got > 1e-5).double().mean().item()
    print("%s: max err vs f64 truth: hip %.3g, f32 reference %.3g; frac > 1e-5: %.5f; median %.3g; rows %d"
          % (name, e_got.max(), e_ref.max(), frac, e_got.median(), e_got.numel()))
    assert e_got.max().item() <= 3 * e_ref.max().item() + 2e-6, (name, e_got.max().item(), e_ref.max().item())
    assert frac < 0.01 and e_got.median().item() < 1e-6, (name, frac, e_got.median().item())


def ulp_distance(a, b):
    """Elementwise distance of two float32 tensors in units in the last place (both finite, same sign or zero)."""
    ia = a.contiguous().view(torch.int32).long()
    ib = b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return (ia - ib).abs()


def kernel_tangent_frame(normals):
    """The isotropic kernel's deterministic tangent frame (csrc/splat.hip, splat_setup_point), operation by operation in
    float32 so that it is reproduced to the bit: e = the axis least aligned with n (first on ties: x, then y),
    u = normalize(n x (n + e)), v = normalize(n x u).  Returns u, v (P,3)."""
    n = normals.float()
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    ax, ay, az = nx.abs(), ny.abs(), nz.abs()
    is_x = (ax <= ay) & (ax <= az)
    is_y = ~is_x & (ay <= az)
    is_z = ~is_x & ~is_y
    mx, my, mz = nx + is_x.float(), ny + is_y.float(), nz + is_z.float()

    def cross_unit(bx, by, bz):
        cx, cy, cz = ny * bz - nz * by, nz * bx - nx * bz, nx * by - ny * bx
        norm = torch.sqrt((cx * cx + cy * cy) + cz * cz).clamp(min=1e-12)
        return cx / norm, cy / norm, cz / norm

    u = cross_unit(mx, my, mz)
    v = cross_unit(*u)
    return torch.stack(u, -1), torch.stack(v, -1)
