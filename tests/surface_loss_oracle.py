"""Oracle of the point regularisers (include/isopoints.h section K; iso_points_amd.loss.surface_losses): torch on the CPU,
written from the formulas of the header, one cloud at a time, with a dtype switch.  The float64 run is the reference; the
float32 run of the same lines is what the tests derive their tolerances from.

    cloud(P, seed)                 the test clouds: a jittered unit sphere with noisy, unnormalised normals
    lattice(n, a, lifted, h)       a planar lattice with one point lifted along the common normal
    knn_others(points, K)          brute force: the K nearest other points of every point, float64 distances
    sweeps(...)                    n1, n2, both losses through torch ops (autograd reaches `points`), the closed-form
                                   gradients, and what the comparison rules need (ball margins, weight sums)
"""
import math

import torch

EPS_DENOM = 1e-17


def cloud(P, seed):
    """(points (P,3), normals (P,3)) float32: unit sphere, radial jitter sigma = 0.02, normals = position + 0.3 noise,
    left unnormalised."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(P, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    pts = d * (1.0 + 0.02 * torch.randn(P, 1, generator=g, dtype=torch.float64))
    nrm = pts + 0.3 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    return pts.float(), nrm.float()


def lattice(n, a, lifted, h):
    """(points (n*n,3), normals (n*n,3)) float32: the lattice a * (i, j, 0), every normal (0, 0, 1), point `lifted` raised by
    h.  With a and h powers of two every coordinate and every squared distance is exact in float32."""
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    pts = torch.stack([ii.reshape(-1) * a, jj.reshape(-1) * a, torch.zeros(n * n)], dim=-1).float()
    pts[lifted, 2] = h
    nrm = torch.zeros(n * n, 3)
    nrm[:, 2] = 1.0
    return pts, nrm


def pair_d2(points):
    """(P,P) float64 squared distances of float32 points."""
    p = points.double()
    return (p[:, None, :] - p[None, :, :]).square().sum(dim=-1)


def knn_others(points, K, extra=0):
    """Brute force in float64: (dists (P,K+extra), idx (P,K+extra)) of the nearest OTHER points, ascending by (d2, index)."""
    d2 = pair_d2(points)
    d2.fill_diagonal_(float("inf"))
    val, idx = torch.sort(d2, dim=1, stable=True)
    return val[:, :K + extra], idx[:, :K + extra]


def dists_f32(points, idx):
    """The squared distances as the search computes them: (dx*dx + dy*dy) + dz*dz in float32."""
    d = points.float()[:, None, :] - points.float()[idx]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def eps_denom(x):
    sign = x.sign() + (x == 0).to(x.dtype)
    return sign * x.abs().clamp_min(EPS_DENOM)


def unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def phi(dists, fs):
    s = ((dists[:, :1] * 2.0) * fs) * fs
    w = (1.0 - dists / s).clamp_min(0.0)
    w = w * w
    return w * w


def normal_w(nrm, idx, inv_sigma2):
    u = unit(nrm)
    d = u[idx] - u[:, None, :]
    return torch.exp(-d.square().sum(dim=-1) * inv_sigma2)


def mollify(nrm, idx, w):
    return (nrm[idx] * w[..., None]).sum(dim=-2) / eps_denom(w.sum(dim=-1, keepdim=True))


def sweeps(points, normals, idx, dists, fs=2.0, sigma=0.75, dtype=torch.float64, nbr_points=None, bandwidth=None):
    """One cloud without padding: points, normals (L,3), idx (L,K) int64, dists (L,K).  nbr_points: the positions the lists
    were built on (default: the points, detached).  `points` may require grad (in `dtype`): proj / rep are built from
    torch ops on it; everything else is a constant, as in the reference.  Returns a dict:
      n1, n2 (L,3); proj, rep (L,); gproj, grep (L,3) the closed forms of the header;
      sum_w, sum_W (L,) the two weight sums; margin (L,) the smallest |d_k / (2 fs d_0) - 1| of the row."""
    L, K = idx.shape
    p = points.to(dtype)
    pd = p.detach()
    x = (pd if nbr_points is None else nbr_points.to(dtype))[idx]                     # (L,K,3) constants
    n0 = normals.to(dtype)
    d = dists.to(dtype)
    inv_sigma2 = 1.0 / (sigma * sigma)
    bw = (L / 2.0) if bandwidth is None else bandwidth
    ph = phi(d, fs)
    n1 = mollify(n0, idx, ph)
    nu = normal_w(n1, idx, inv_sigma2)
    n2 = mollify(n1, idx, ph * nu)
    ball = d > (fs * d[:, :1]) * 2.0
    w = (ph * nu).masked_fill(ball, 0.0)
    m = n2[idx]                                                                      # (L,K,3)
    den_w = eps_denom(w.sum(dim=-1))

    def project(pp):
        s = ((x - pp[:, None, :]) * m).sum(dim=-1)
        D = (w * s).sum(dim=-1) / den_w
        q = pp + ((s * w)[..., None] * m).sum(dim=-2) / den_w[:, None]
        return s, D, q
    s, D, q = project(p)
    proj = D * D
    with torch.no_grad():
        e2_const = (x - q[:, None, :]).square().sum(dim=-1)
        sig = torch.exp(-e2_const * bw)
        dens = sig.sum(dim=-1, keepdim=True) + 1.0
        W = ((nu * sig) * dens).masked_fill(ball, 0.0)
        den_W = eps_denom(W.sum(dim=-1))
    e = q[:, None, :] - x
    rep = -((e * e).sum(dim=-1) * W).sum(dim=-1) / den_W
    with torch.no_grad():
        a = (w[..., None] * m).sum(dim=-2) / den_w[:, None]
        gproj = (2.0 * D.detach())[:, None] * -a
        ed = e.detach()
        g = -((2.0 * ed) * W[..., None]).sum(dim=-2) / den_W[:, None]
        mg = w * (m * g[:, None, :]).sum(dim=-1)
        grep = g - (mg[..., None] * m).sum(dim=-2) / den_w[:, None]
        margin = (dists.double() / (2.0 * fs * dists.double()[:, :1]) - 1.0).abs().min(dim=-1).values
    return dict(n1=n1, n2=n2, proj=proj, rep=rep, gproj=gproj, grep=grep, sum_w=w.sum(dim=-1), sum_W=W.sum(dim=-1),
                margin=margin)


def tolerance(f32, ref):
    """A = 4 x the largest error of the oracle's float32 run against its float64 run, the error taken as at least half a
    float32 step at the largest reference entry (so A >= two steps).  Returns (A, measured error)."""
    err = (f32.detach().double() - ref.detach().double()).abs().max().item() if ref.numel() else 0.0
    top = ref.detach().abs().max().item() if ref.numel() else 0.0
    half_step = 0.5 * 2.0 ** (math.floor(math.log2(top)) - 23) if top > 0 else 0.0
    return 4.0 * max(err, half_step), err


def assert_plane_normal(n):
    """n is (0, 0, 1): x and y exactly (sums of zeros); z = sum(w * 1) / sum(w) with the two sums of K = 32 positive terms
    possibly added in different orders, each within 31 roundings of 2^-24, once per mollification: within 8e-6 of 1."""
    n = n.detach().cpu().double()
    assert n[0].item() == 0.0 and n[1].item() == 0.0 and abs(n[2].item() - 1.0) <= 8e-6, n
