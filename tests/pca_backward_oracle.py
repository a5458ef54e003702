"""Oracle of the local-frame estimator's backward pass (iso_pca_frames_backward); a helper, not a test.

  frames_fixed   the contract of iso_pca_frames as a differentiable torch expression on ONE cloud (L,3) with a given
                 neighbour index: eigh of the centred neighbourhood covariance, ascending, clamped at 0, with the sign of
                 every eigenvector fixed as a constant (aligned with reference frames, e.g. the ones the GPU returned), and
                 with `disambiguate` the frame (n, n x z, z).  torch autograd through it is the judge in float64 and, in
                 float32, the yardstick the kernel's error is measured by.
  closed_form    the adjoint the kernels implement, with this package's rules (pairs within 2e-5 lambda_max exchange
                 nothing, lambda_max = 0 gives 0, an eigenvalue that is 0 passes nothing), in any float type.
  normal_loss    the three lines of NormalLoss.compute (DSS/training/losses.py:98-102) on frames_fixed.
  errors / judge the two norms of the issue and the 10 x rule.
"""
import numpy as np
import torch

GAP_RULE = 2e-5          # the kernel's rule: |l_b - l_a| <= GAP_RULE * l_max exchanges nothing
WELL_SEPARATED = 1e-2    # rows judged on their eigenvectors: every needed gap >= this times l_max (tests/test_pca_cpu.py::judge)
FACTOR = 10.0            # the kernel's error may be at most this many times the float32 yardstick's


def neighbourhoods(x, idx):
    """Centred neighbours D (R,K,3) and covariances C (R,3,3) of rows with neighbour indices idx (R,K) in cloud x (L,3)."""
    X = x[idx]
    D = X - X.mean(dim=1, keepdim=True)
    return D, torch.einsum("rki,rkj->rij", D, D) / idx.shape[1]


def _aligned(U, ref_frames, disambiguate):
    """U's columns with the constant signs that align them with ref_frames (None: as they are); with `disambiguate` the
    frame (n, n x z, z)."""
    if ref_frames is None:
        s = torch.ones(U.shape[0], 3, dtype=U.dtype)
    else:
        dots = (U.detach() * ref_frames.to(U.dtype)).sum(dim=1)                  # (R,3): <u_c, ref_c>
        s = torch.where(dots < 0, -torch.ones_like(dots), torch.ones_like(dots))
    if not disambiguate:
        return U * s[:, None, :]
    n, z = U[:, :, 0] * s[:, 0:1], U[:, :, 2] * s[:, 2:3]
    return torch.stack([n, torch.cross(n, z, dim=1), z], dim=2)


def frames_fixed(x, idx, ref_frames=None, disambiguate=False):
    """(curvature (R,3), frames (R,3,3)) of one cloud, differentiable w.r.t. x; signs constant."""
    _, C = neighbourhoods(x, idx)
    w, U = torch.linalg.eigh(C)
    return w.clamp(min=0), _aligned(U, ref_frames, disambiguate)


def autograd_grad(x, idx, ref_frames, disambiguate, g_l, g_V, dtype=torch.float64):
    """d [sum(g_l * curvature) + sum(g_V * frames)] / dx by torch autograd through frames_fixed, in `dtype`."""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    w, F = frames_fixed(xx, idx, ref_frames, disambiguate)
    loss = (w * g_l.to(dtype)).sum() + (F * g_V.to(dtype)).sum()
    (g,) = torch.autograd.grad(loss, xx)
    return g


def closed_form(x, idx, ref_frames, disambiguate, g_l, g_V, dtype=torch.float64):
    """The adjoint of the issue with the package's rules.  Returns (grad (L,3), curvature, frames)."""
    with torch.no_grad():
        x = x.detach().to(dtype)
        g_l, g_V = g_l.to(dtype), g_V.to(dtype)
        K = idx.shape[1]
        D, C = neighbourhoods(x, idx)
        w, U = torch.linalg.eigh(C)
        w = w.clamp(min=0)
        F = _aligned(U, ref_frames, disambiguate)
        if disambiguate:
            n, z, gy = F[:, :, 0], F[:, :, 2], g_V[:, :, 1]
            gn = g_V[:, :, 0] + torch.cross(z, gy, dim=1)
            gz = g_V[:, :, 2] + torch.cross(gy, n, dim=1)
            gv = torch.stack([gn, torch.zeros_like(gn), gz], dim=2)
        else:
            gv = g_V
        M = torch.einsum("rka,rkb->rab", F, gv)                                  # M_ab = v_a . gv_b
        gap = w[:, None, :] - w[:, :, None]                                      # gap_ab = l_b - l_a
        lmax = w.max(dim=1).values
        ok = gap.abs() > GAP_RULE * lmax[:, None, None]
        S = torch.where(ok, (M - M.transpose(1, 2)) / (2 * torch.where(ok, gap, torch.ones_like(gap))), torch.zeros_like(M))
        dl = torch.where(w > 0, g_l, torch.zeros_like(g_l))
        G = torch.einsum("rab,rbc,rdc->rad", F, torch.diag_embed(dl) + S, F)
        contrib = (2.0 / K) * torch.einsum("rab,rkb->rka", G, D)
        grad = torch.zeros_like(x).index_add_(0, idx.reshape(-1), contrib.reshape(-1, 3))
    return grad, w, F


def min_gap(w, columns):
    """Per row the smallest gap, relative to l_max, between eigenvalue c (c in columns) and any other eigenvalue."""
    w = np.asarray(w, dtype=np.float64)
    lmax = np.maximum(w.max(axis=1), 1e-300)
    gaps = []
    for c in columns:
        for o in range(3):
            if o != c:
                gaps.append(np.abs(w[:, c] - w[:, o]))
    return np.min(np.stack(gaps, 0), axis=0) / lmax


def normal_loss(x, normals, idx, ref_frames=None):
    """1 - |cos(normals, PCA normal)| per point of one cloud (the sign of the PCA normal does not matter)."""
    _, F = frames_fixed(x, idx, ref_frames, False)
    return 1 - torch.nn.functional.cosine_similarity(normals, F[:, :, 0]).abs()


def errors(g, g64):
    """(relative L2 over the cloud, max|g - g64| / max|g64|)."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return (float(np.linalg.norm(g - g64) / np.linalg.norm(g64)), float(np.abs(g - g64).max() / np.abs(g64).max()))


def judge(got, yard, g64, what):
    """The rule of the backward's tests: the kernel's error against float64 is at most FACTOR x the error of the float32
    torch evaluation of the same restatement, in both norms.  Prints both and the ratios; returns the ratios."""
    assert np.isfinite(np.asarray(got)).all(), "%s: non-finite gradient" % what
    e_k, e_y = errors(got, g64), errors(yard, g64)
    ratios = tuple(k / max(y, 1e-300) for k, y in zip(e_k, e_y))
    print("%s: kernel rel-L2 %.3e max %.3e | float32 yardstick rel-L2 %.3e max %.3e | ratios %.2f %.2f"
          % (what, e_k[0], e_k[1], e_y[0], e_y[1], ratios[0], ratios[1]))
    assert e_k[0] <= FACTOR * e_y[0] and e_k[1] <= FACTOR * e_y[1], \
        "%s: kernel error (%.3e, %.3e) beyond %g x the float32 yardstick (%.3e, %.3e)" % (what, e_k[0], e_k[1], FACTOR,
                                                                                             e_y[0], e_y[1])
    return ratios


# ------------------------------------------------------------------------------------------------ the tests' clouds
def noisy_sphere(P, jitter, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
    return (p + jitter * (torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5)).float()


def cube_surface(P, jitter, seed):
    """Points on the surface of [-1, 1]^3 (faces, edges and corners), as tests/golden/make_golden_pca.py draws them."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(P, 3, generator=g, dtype=torch.float64) * 2 - 1
    face = torch.randint(0, 6, (P,), generator=g)
    u[torch.arange(P), face % 3] = (face // 3).double() * 2 - 1
    return (u + jitter * (torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5)).float()


def brute_knn(x, K):
    """Exact kNN index (L,K) of a small cloud, the point itself included, ties to the lower index (float64 distances)."""
    x = x.double()
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return torch.sort(d2, dim=1, stable=True).indices[:, :K].contiguous()


def incoming(R, seed, w, columns):
    """Random incoming gradients g_l (R,3) on all eigenvalues and g_V (R,3,3) on `columns`, g_V zeroed on rows where a gap
    those columns need is below WELL_SEPARATED * l_max.  Returns (g_l, g_V, share of rows zeroed)."""
    g = torch.Generator().manual_seed(seed)
    g_l = torch.randn(R, 3, generator=g, dtype=torch.float64)
    g_V = torch.randn(R, 3, 3, generator=g, dtype=torch.float64)
    keep = torch.zeros(3, dtype=torch.float64)
    keep[list(columns)] = 1.0
    g_V = g_V * keep[None, None, :]
    # with the sign rule column 1 = n x z pulls on columns 0 and 2: the needed gaps are those of the columns it touches
    need = set(columns) | ({0, 2} if 1 in columns else set())
    bad = torch.from_numpy(min_gap(w, sorted(need)) < WELL_SEPARATED)
    g_V[bad] = 0.0
    return g_l, g_V, float(bad.double().mean())
