"""float64 statements of the densify stage (csrc/repulse.hip, csrc/insert.hip), their acceptance criteria, and the input
sets that tests/test_densify_cpu.py and tests/test_densify_gpu.py share.  No GPU and no iso_points_amd import here.

The five operations, written from the reference statements the kernel headers cite:

  upsample candidates   DSS/utils/point_processing.py:326-339        upsample_scores
  EAR candidates        DSS/models/levelset_sampling.py:609-628      ear_scores
  repulsion             DSS/models/levelset_sampling.py:268-284      repulse
  insert                DSS/models/levelset_sampling.py:200-218      fathers, children, insert

Every criterion takes the kernel's float32 output and this module's float64 values; u = 2^-24 is the unit roundoff of
float32 (one correctly rounded operation: relative error <= u).  The library is built without contraction and with
correctly rounded division and square root; a square root is allowed 2 u all the same.  Bounds are first order in u and
every constant is rounded up, which covers the higher orders at the magnitudes used.  None of the constants was set
by looking at what a kernel returns; the one measured allowance (powf) is measured on the CPU, see A_POW.

CANDIDATES (check_candidates).  The candidate of a row is an arg-max, and float32 cannot reproduce a float64 arg-max
at near-ties, so the criterion is a fence.  The float32 midpoints mid_k = (nn_k + 2 p) / 3 are the same bits on any
IEEE machine: mids_f32 computes them on the CPU and the kernel's candidate must equal one of them bit for bit (the
lowest column where several are identical; columns with one midpoint have one upsample score, but their EAR scores
differ with their normals, and there it is the lowest of those that score highest).  With s_k the float64 score of
column k and e_k a bound on |float32 score - s_k|, the chosen column c must satisfy  s_c + e_c >= max_k (s_k - e_k)
and the returned sparsity  |sparsity - s_c| <= e_c.  (Where e is the same for every column this reads "s_c >= max s - 2 e".)

  upsample, e = C_UPS u S = 20 u S for every column of a row, S = the row's largest |coordinate| (point and
  neighbours; every midpoint has |coordinate| <= S):
    - mid_k: two roundings (the sum, the division; 2 p is exact), so |mid32 - mid64| <= 2 u S per component,
      2 sqrt(3) u S < 3.5 u S as a vector, and a distance moves by at most that;
    - per (k, j) pair, from exact inputs: three subtractions (u each), three squares (2 u carried + u), two adds
      (2 u): 5 u on the squared distance, 2.5 u after the root, + 2 u for the root itself = 4.5 u relative to a
      distance D <= 2 sqrt(3) S, so < 15.6 u S;
    - min and max select and add nothing: 3.5 + 15.6 = 19.1, rounded up to 20.

  EAR, e_k per column (the score takes a square root of a difference that can be near zero, so no single multiple
  of the row's score scale is a bound; each term below is a constant times u times a scale of the row).  With S as
  above, D the row's largest float64 |mid_k - nn_j| and U the row's largest |neighbour-normal component|:
    - |d|: 4.5 u D + 3.5 u S as above;
    - q = sum_c (d_c u_c)^2: d_c carries 2 u S (midpoint) + u |d_c| (subtraction); the product with u_c adds u, the
      square 2 x carried + u, the two adds 2 u q:  <= u U^2 (4 sqrt(3) D S + 5 D^2 + 2 D^2) <= u U^2 (7 D S + 7 D^2);
    - v = |d| - q: + u |v| <= u (D + U^2 D^2).  So |v32 - v64| <= E_v = u (3.5 S + 5.5 D + U^2 (7 D S + 8 D^2)), and
      min_j, |.| and the clamp at 1e-17 (the float32 constant, in both) do not enlarge it;
    - m = sqrt(x): |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt(|a - b|)), + 2 u m for the root:
      e_m = min(E_v / m, sqrt(E_v)) + 2 u m;
    - g = 2 - n . u_k: three products and two adds carry 3 u sum_c |n_c u_c|, the subtraction u |g|:
      e_g = u (3 sum_c |n_c u_c| + |g|);  edge = g (edge_sensitivity 1: e_edge = e_g),  g g (2: 2 |g| e_g + u g^2),
      else powf(g, s): edge (|s| e_g / |g| + A_POW u);
    - score = edge m: e_k = 1.001 (e_edge m + edge e_m + u edge m)   (1.001: the product of the two errors).
  A_POW = 2.14: torch.pow in float32 against float64 on 4e6 bases in [1, 3] and exponents 0.5, 1.5, 2.5 (the float32
  CPU restatement's own call) is off by at most 1.07 u relative; doubled.  test_densify_cpu.py measures it again.

  Tie rule (exact=True).  On the lattice inputs (coordinates 3 h a, h = 2^-6, a small integers; axis-aligned normals;
  edge_sensitivity 1 or 2) every midpoint, squared distance, squared product and edge factor is exact in float32
  and two columns either tie in both precisions or differ by far more than a rounding, so the fence does not apply:
  the chosen column must be the FIRST float64 maximum.  The sparsity keeps the bound above.

REPULSE (check_repulse).  The project's standing criterion (tests/test_resample_gpu.py):
|out - ref|.max() / |ref - p|.max() < 1e-5 against float64; rows whose float64 move is exactly zero (all neighbours
-1, K == 0, every weight underflowed) must come back bit-equal to the input point; the output is finite everywhere.

FATHERS (check_fathers).  father = (0 < d2 < params[1]) and (d2 < params[0]), d2 the squared distance to the nearest
of the first n_refs reference points.  Per reference point: three subtractions (u), three squares (2 u + u), two adds
(2 u) = 5 u relative on d2, C_FATHERS = 6 with the higher orders; the minimum over reference points keeps it.  A row
is inside the fence when |d2 - params[i]| <= 6 u d2 for i = 0 or 1; at 0 there is no fence (a float32 difference is zero
exactly when the operands are equal).  Outside the fence the mask must match exactly; check_fathers returns the
fenced share, which must stay <= max_fenced (1 % for random inputs, 0 for the dyadic ones).

CHILDREN (check_children).  child(rank, k) = 2 f / 3 + m_k / 3 over the LAST `patch` columns of the index list, a
missing neighbour counting as the origin, at row out_first[b] + (rank - 1) patch + k; rel_err < 1e-6 (the existing
insert tolerance) over the owned rows, and every other row of the output keeps its sentinel bits.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
C_UPS = 20.0
A_POW = 2.14            # 2 x 1.07 (measured, see above)
C_FATHERS = 6.0
CLAMP32 = float(np.float32(1.0e-17))
NORM_EPS32 = float(np.float32(1.0e-12))
REPULSE_TOL = 1e-5
CHILD_TOL = 1e-6
SENTINEL = -7.25


def _bits(x):
    return x.contiguous().view(torch.int32)


def _row_chunks(n, K):
    step = max(1, (1 << 20) // (K * K))
    for s in range(0, n, step):
        yield slice(s, min(n, s + step))


# ----------------------------------------------------------------------------------------------- candidates
def mids_f32(pts, knn):
    """(n,3), (n,K,3) float32 -> the float32 midpoints (n,K,3), operation for operation as the kernels form them
    (numpy: an IEEE addition and division per element)."""
    p, q = pts.detach().cpu().float().numpy(), knn.detach().cpu().float().numpy()
    return torch.from_numpy((q + np.float32(2.0) * p[:, None, :]) / np.float32(3.0))


def upsample_scores(pts, knn):
    """float64 spars_k = min_j |mid_k - nn_j| (n,K) and the bound e (n,K) of the module docstring."""
    n, K = knn.shape[:2]
    score = torch.empty((n, K), dtype=torch.float64)
    p, q = pts.double(), knn.double()
    for r in _row_chunks(n, K):
        mid = (q[r] + 2 * p[r, None, :]) / 3
        score[r] = (mid[:, :, None, :] - q[r, None, :, :]).norm(dim=-1).min(dim=-1).values
    S = torch.maximum(p.abs().amax(-1), q.abs().amax((-1, -2)))
    return score, (C_UPS * U32 * S)[:, None].expand(n, K)


def ear_scores(pts, nrm, knn, knn_n, sens):
    """float64 edge_k m_k (n,K) of levelset_sampling.py:609-628 and the per-column bound e_k (n,K)."""
    n, K = knn.shape[:2]
    sens = float(sens)
    score = torch.empty((n, K), dtype=torch.float64)
    err = torch.empty((n, K), dtype=torch.float64)
    p, nv, q, u = pts.double(), nrm.double(), knn.double(), knn_n.double()
    for r in _row_chunks(n, K):
        mid = (q[r] + 2 * p[r, None, :]) / 3
        d = mid[:, :, None, :] - q[r, None, :, :]                               # (c,K,K,3): [k][j]
        dist = d.norm(dim=-1)
        v = dist - ((d * u[r, :, None, :]) ** 2).sum(dim=-1)                    # the normal of neighbour k, over j
        m = v.min(dim=-1).values.abs().clamp_min(CLAMP32).sqrt()
        g = 2 - (nv[r, None, :] * u[r]).sum(dim=-1)
        edge = g if sens == 1.0 else (g * g if sens == 2.0 else g ** sens)
        score[r] = edge * m
        S = torch.maximum(p[r].abs().amax(-1), q[r].abs().amax((-1, -2)))[:, None]
        D = dist.amax((-1, -2))[:, None]
        U2 = (u[r].abs().amax((-1, -2)) ** 2)[:, None]
        E_v = U32 * (3.5 * S + 5.5 * D + U2 * (7 * D * S + 8 * D * D))
        e_m = torch.minimum(E_v / m, E_v.sqrt()) + 2 * U32 * m
        e_g = U32 * (3 * (nv[r, None, :] * u[r]).abs().sum(dim=-1) + g.abs())
        if sens == 1.0:
            e_edge = e_g
        elif sens == 2.0:
            e_edge = 2 * g.abs() * e_g + U32 * g * g
        else:
            e_edge = edge * (abs(sens) * e_g / g.abs() + A_POW * U32)
        err[r] = 1.001 * (e_edge * m + edge * e_m + U32 * edge * m)
    return score, err


def chosen_columns(pts, knn, cand, score=None):
    """The column whose float32 midpoint equals the candidate bit for bit, -1 where none does.  Where several columns
    have that midpoint (duplicate neighbours) the candidate cannot say which was meant: the lowest of them -- with
    `score`, the lowest of those with the highest score (EAR columns with one midpoint differ by their normals)."""
    same = (_bits(mids_f32(pts, knn)) == _bits(cand.float())[:, None, :]).all(dim=-1)
    if score is not None:
        among = torch.where(same, score, torch.full_like(score, -float("inf")))
        same = same & (among == among.amax(dim=-1, keepdim=True))
    col = same.int().argmax(dim=-1)
    return torch.where(same.any(dim=-1), col, torch.full_like(col, -1))


def first_maximum(score):
    return (score == score.amax(dim=-1, keepdim=True)).int().argmax(dim=-1)


def check_candidates(score, err, pts, knn, sparsity, cand, exact=False):
    """The candidate criterion of the module docstring; sparsity (n,), cand (n,3) from the code under test."""
    sparsity, cand = sparsity.detach().cpu().reshape(-1), cand.detach().cpu().reshape(-1, 3)
    n = score.shape[0]
    assert sparsity.shape[0] == n and cand.shape[0] == n
    assert bool(torch.isfinite(sparsity).all()) and bool(torch.isfinite(cand).all())
    col = chosen_columns(pts, knn, cand, score)
    assert bool((col >= 0).all()), "%d of %d candidates are no float32 midpoint of their row (first row %d)" % (
        int((col < 0).sum()), n, int((col < 0).nonzero()[0]))
    s_c = score.gather(1, col[:, None])[:, 0]
    e_c = err.gather(1, col[:, None])[:, 0]
    if exact:
        want = first_maximum(score)
        bad = col != want
        assert not bool(bad.any()), "%d of %d rows do not take the first maximum (row %d: column %d, first maximum %d)" % (
            int(bad.sum()), n, int(bad.nonzero()[0]), int(col[bad][0]), int(want[bad][0]))
    else:
        short = (score - err).amax(dim=-1) - (s_c + e_c)
        bad = short > 0
        assert not bool(bad.any()), "%d of %d rows chose a column below the float64 maximum by more than the margin " \
            "(row %d: short by %.3g, margin %.3g)" % (int(bad.sum()), n, int(short.argmax()), float(short.max()),
                                                       float(e_c[short.argmax()]))
    off = (sparsity.double() - s_c).abs() - e_c
    assert float(off.max()) <= 0, "sparsity off its column's float64 score by %.3g beyond the margin %.3g (row %d)" % (
        float(off.max()), float(e_c[off.argmax()]), int(off.argmax()))


def candidate_inputs(kind, n, K, seed=0):
    """pts (n,3), nrm (n,3), knn (n,K,3), knn_n (n,K,3), float32.
    jitter  neighbours = point + 0.05 randn, normals around the point's (the suite's existing inputs)
    equal   every neighbour IS the point (score 0)
    padded  jitter with trailing columns (and whole rows) zeroed in positions and normals, as frnn_gather returns -1
    lattice coordinates 3 h a (h = 2^-6, integer a), offsets in {-2..2}^3, axis-aligned normals: exact ties"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * K + n % 997)
    if kind == "lattice":
        h = 2.0 ** -6
        pts = 3 * h * torch.randint(-8, 9, (n, 3), generator=g).float()
        knn = pts[:, None, :] + 3 * h * torch.randint(-2, 3, (n, K, 3), generator=g).float()

        def axis(shape):
            a = torch.nn.functional.one_hot(torch.randint(0, 3, shape, generator=g), 3).float()
            return a * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)[..., None]
        return pts, axis((n,)), knn, axis((n, K))
    pts = torch.rand(n, 3, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    knn = pts[:, None, :] + 0.05 * torch.randn(n, K, 3, generator=g)
    knn_n = torch.nn.functional.normalize(nrm[:, None, :] + 0.5 * torch.randn(n, K, 3, generator=g), dim=-1)
    if kind == "equal":
        knn, knn_n = pts[:, None, :].expand(n, K, 3).contiguous(), nrm[:, None, :].expand(n, K, 3).contiguous()
    elif kind == "padded":
        knn[::3, K - (K + 2) // 3:] = 0
        knn_n[::3, K - (K + 2) // 3:] = 0
        knn[::10] = 0
        knn_n[::10] = 0
    else:
        assert kind == "jitter"
    return pts, nrm, knn, knn_n


SECOND_SWEEP_64 = 4096 * 64 + 65          # iso_stream_grid caps a launch at 4096 workgroups; 64 lanes each
SECOND_SWEEP_256 = 4096 * 256 + 257
# (kind, n, K): the row counts, the list sizes at n = 1000, the input kinds
CANDIDATE_CASES = [("jitter", n, 16) for n in (1, 63, 64, 65, 2000)] + [("jitter", SECOND_SWEEP_64, 2)] + \
    [("jitter", 1000, K) for K in (1, 2, 16, 31, 32, 33, 42, 43, 64)] + \
    [("equal", 1000, 16), ("padded", 1000, 16), ("padded", 300, 1)]
LATTICE_CASES = [("lattice", 1000, K) for K in (1, 2, 16, 31, 64)] + [("lattice", SECOND_SWEEP_64, 2)]
EAR_SENS = (1.0, 2.0, 1.5, 0.5)


def ear_case_list():
    """(kind, n, K, edge_sensitivity, exact) for every EAR run."""
    out = [(k, n, K, 1.0, False) for k, n, K in CANDIDATE_CASES]
    out += [("jitter", 2000, 16, s, False) for s in EAR_SENS[1:]] + [("jitter", 1000, 64, 1.5, False),
                                                                     ("padded", 1000, 16, 0.5, False)]
    out += [(k, n, K, s, True) for k, n, K in LATTICE_CASES for s in (1.0, 2.0)]
    return out


def upsample_case_list():
    return [(k, n, K, False) for k, n, K in CANDIDATE_CASES] + [(k, n, K, True) for k, n, K in LATTICE_CASES]


# ----------------------------------------------------------------------------------------------- repulse
def eps_denom64(x, eps=1e-17):
    sign = torch.sign(x) + (x == 0).to(x.dtype)
    return sign * x.abs().clamp_min(eps)


def repulse(pts, nrm, idx, inv_sigma, first=0):
    """float64 levelset_sampling.py:268-284 for the rows first .. first + n of one cloud: pts, nrm (P,3) float32 (normals
    un-normalised: F.normalize, v / max(|v|, 1e-12)), idx (n,K) int64 into the cloud, -1 = missing."""
    n, K = idx.shape
    p = pts.double()
    rows = p[first:first + n]
    if K == 0:
        return rows.clone()
    safe = idx.clamp(min=0)
    q = p[safe]
    u = nrm.double()[safe]
    u = u / u.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS32)
    d = rows[:, None, :] - q
    w = torch.exp(-(d * d).sum(dim=-1) * float(inv_sigma))
    w = torch.where(idx < 0, torch.zeros_like(w), w)
    t = d - (d * u).sum(dim=-1, keepdim=True) * u
    sw = w.sum(dim=-1, keepdim=True)
    return rows + (sw + 1.0) * (w[..., None] * t).sum(dim=-2) / eps_denom64(sw)


def check_repulse(pts, ref, out, first=0):
    """ref = repulse(...) (n,3) float64; out (n,3) float32 from the code under test."""
    out = out.detach().cpu().reshape(-1, 3)
    n = ref.shape[0]
    assert out.shape[0] == n and bool(torch.isfinite(out).all())
    rows = pts[first:first + n]
    move = ref - rows.double()
    still = (move == 0).all(dim=-1)
    moved_bits = (out[still] != rows[still]).any(dim=-1)
    assert not bool(moved_bits.any()), "%d of %d rows with a zero float64 move came back changed" % (
        int(moved_bits.sum()), int(still.sum()))
    if float(move.abs().max()) > 0:
        e = float((out.double() - ref).abs().max() / move.abs().max())
        assert e < REPULSE_TOL, "repulsion off by %.3g of the largest move (tolerance %g)" % (e, REPULSE_TOL)
    return int(still.sum())


def repulse_inputs(P, K, seed=0, degenerate=True):
    """A jittered helix on the unit sphere whose neighbours along the curve are about sqrt(diag / P) apart, so that
    exp(-d^2 P / diag) is of order one for the nearest: pts, nrm (P,3) (un-normalised normals), the (P, K + 1) index
    list [self, +1, -1, +2, -2, ...] with -1 past the ends, and inv_sigma = P / diag as float32.  `degenerate` adds
    scattered -1, rows of all -1 and rows of zero normals.  Past 5000 points the spacing and inv_sigma stay those of
    5000: the float32 coordinates of a unit cloud carry 2^-24, the standing criterion measures the error against the
    largest move, and a move of 1e-3 (the spacing of a million points) would leave it no room."""
    g = torch.Generator().manual_seed(seed + P)
    t = (torch.arange(P, dtype=torch.float64) + 0.5) / P
    z = 1 - 2 * t
    rad = (1 - z * z).sqrt()
    dense = min(P, 5000)
    phi = t * P * math.sqrt(3.5 / dense) / 0.8
    pts = torch.stack([rad * phi.cos(), rad * phi.sin(), z], dim=-1).float()
    pts = pts + (0.3 / math.sqrt(dense)) * (torch.rand(P, 3, generator=g) - 0.5)
    nrm = pts * 1.7 + 0.1 * torch.randn(P, 3, generator=g)
    i = torch.arange(P)[:, None]
    steps = torch.tensor([0] + [(m // 2 + 1) * (1 if m % 2 == 0 else -1) for m in range(K)])[None, :]
    idx = i + steps
    idx = torch.where((idx < 0) | (idx >= P), torch.full_like(idx, -1), idx)
    if degenerate:
        idx[::7, -2:] = -1
        idx[5::11, 1:] = -1
        nrm[3::13] = 0
    diag = float((pts.max(0).values - pts.min(0).values).norm()) if P > 1 else 1.0
    return pts, nrm, idx, torch.tensor([dense / diag], dtype=torch.float32)


# (P, n, first, K, inv_sigma: None = P / diag): row counts, list sizes, the sharded route, underflowed weights
REPULSE_CASES = [(n, n, 0, 8, None) for n in (1, 255, 256, 257, 5000)] + [(SECOND_SWEEP_256, SECOND_SWEEP_256, 0, 2, None)] + \
    [(1000, 1000, 0, K, None) for K in (0, 1, 31)] + [(5000, 1000, 300, 8, None), (5000, 1000, 0, 8, None),
                                                      (5000, 257, 300, 31, None), (1000, 1000, 0, 8, 1e30),
                                                      (5000, 1000, 300, 8, 1e30)]


# ----------------------------------------------------------------------------------------------- insert
def fathers(pts, lens, refs, n_refs, params):
    """pts (B,P,3) float32, lens (B,) or None, refs (R,3) of which the first n_refs count, params = (r2, lim) float32
    -> float64 mask (B,P) bool, nearest d2 (B,P), fenced (B,P) bool (rows past a cloud's length: never a father,
    never fenced)."""
    B, P = pts.shape[:2]
    r = refs[:int(n_refs)].double()
    d2 = torch.full((B, P), float("inf"), dtype=torch.float64)
    for k in range(r.shape[0]):                                              # (n_refs <= 64: a loop keeps 1e6 rows cheap)
        d2 = torch.minimum(d2, ((pts.double() - r[k]) ** 2).sum(dim=-1))
    r2, lim = float(params[0]), float(params[1])
    valid = torch.ones((B, P), dtype=torch.bool) if lens is None else torch.arange(P)[None, :] < lens.view(-1, 1)
    mask = (d2 > 0) & (d2 < lim) & (d2 < r2) & valid
    tol = C_FATHERS * U32 * d2
    fenced = (((d2 - r2).abs() <= tol) | ((d2 - lim).abs() <= tol)) & valid & torch.isfinite(d2)
    return mask, d2, fenced


def check_fathers(mask, fenced, father, max_fenced=0.01):
    """father (B,P) uint8 from the code under test; returns the fenced share of the rows."""
    father = father.detach().cpu()
    assert father.shape == mask.shape and father.dtype == torch.uint8 and int(father.max()) <= 1
    if max_fenced == 0:                                   # the dyadic cases: no row is excused
        fenced = torch.zeros_like(fenced)
    share = float(fenced.double().mean())
    bad = (father.bool() != mask) & ~fenced
    assert share <= max_fenced and not bool(bad.any()), \
        "fenced share %.4f %% (at most %.2f %%); %d rows outside the fence differ from the float64 mask" % (
            100 * share, 100 * max_fenced, int(bad.sum()))
    return share


def children(pts, knn, father, out_first, patch, n_rows):
    """float64 children in the kernel's row layout: (n_rows,3), NaN where no father owns the row.  pts (B,P,3), knn (B,P,K)
    int64 (-1 = missing -> the origin), father (B,P) bool/uint8, out_first (B,)."""
    B, P, K = knn.shape
    out = torch.full((n_rows, 3), float("nan"), dtype=torch.float64)
    p = pts.double()
    for b in range(B):
        rows = father[b].bool().nonzero().reshape(-1)
        if rows.numel() == 0:
            continue
        nb = knn[b, rows, K - patch:]
        m = p[b][nb.clamp(min=0)] * (nb >= 0)[..., None].double()
        c = 2 * p[b, rows][:, None, :] / 3 + m / 3
        start = int(out_first[b])
        out[start:start + rows.numel() * patch] = c.reshape(-1, 3)
    return out


def check_children(ref, out):
    """ref from children(); out (n_rows,3) float32, SENTINEL-filled before the code under test ran."""
    out = out.detach().cpu()
    assert out.shape == ref.shape
    owned = ~torch.isnan(ref[:, 0])
    keep = _bits(out[~owned]) == _bits(torch.full_like(out[~owned], SENTINEL))
    assert bool(keep.all()), "%d rows that no father owns were written" % int((~keep.all(dim=-1)).sum())
    if bool(owned.any()):
        assert bool(torch.isfinite(out[owned]).all())
        e = float((out[owned].double() - ref[owned]).abs().max() / ref[owned].abs().max().clamp_min(1e-30))
        assert e < CHILD_TOL, "children off by %.3g relative (tolerance %g)" % (e, CHILD_TOL)


def fathers_inputs(P, lens, n_refs, seed=0):
    """A unit-cube cloud (B = len(lens) or 1), 50 reference rows of which n_refs count, limits that make about a third
    of the rows fathers; a few points sit exactly on a reference point, and the rows past a cloud's length are placed
    where they would be fathers."""
    g = torch.Generator().manual_seed(seed + 31 * P + n_refs)
    B = 1 if lens is None else len(lens)
    refs = torch.rand(50, 3, generator=g) * 0.8 + 0.1
    pts = torch.rand(B, P, 3, generator=g)
    pts[:, ::17] = refs[0]
    if P > 40:
        pts[:, 5::40] = refs[:n_refs][torch.randint(0, n_refs, (B, len(range(5, P, 40))), generator=g)]
    lim = 0.25 if n_refs < 10 else 0.02
    params = torch.tensor([0.64 if n_refs < 10 else 0.015, lim], dtype=torch.float32)
    if lens is not None:
        for b, l in enumerate(lens):
            pts[b, l:] = refs[0] + 0.01
    return pts, (None if lens is None else torch.tensor(lens, dtype=torch.int64)), refs, n_refs, params


# (P, lens, n_refs)
FATHERS_CASES = [(P, None, r) for P in (1, 255, 257) for r in (1, 50)] + [(1000, [1000, 700, 0], 50), (1000, [1000, 700, 0], 1),
                                                                         (SECOND_SWEEP_256, None, 3)]


def fathers_dyadic():
    """Points exactly on a reference point, exactly at d2 = a limit, one ulp inside and one ulp outside, for each of the
    two limits binding in turn: [(pts (1,P,3), refs, n_refs, params)].  Every d2 is one exact square (the offset lies
    along an axis), so float32 and float64 agree and no fence is allowed."""
    out = []
    refs = torch.tensor([[0.0, 0.0, 0.0], [4.0, 4.0, 4.0]])           # (the origin: point = offset, no rounding)
    for params in ((1.0, 0.0625), (0.0625, 1.0), (0.0625, 0.0625)):
        r = np.float32(0.25)
        offs = [0.0, r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(1)), np.float32(0.125), np.float32(0.5)]
        rows = []
        for axis in range(3):
            for sgn in (1.0, -1.0):
                for o in offs:
                    p = refs[0].clone()
                    p[axis] = p[axis] + sgn * float(o)
                    rows.append(p)
        out.append((torch.stack(rows)[None], refs, 2, torch.tensor(params, dtype=torch.float32)))
    return out


def children_inputs(P, lens, K, seed=0, patch=8):
    """pts (B,P,3), an index list (B,P,K) with scattered -1 and rows of all -1, a father mask that respects the
    lengths, its inclusive rank, out_first with a gap of three rows before every cloud, and the row count (three spare
    rows at the end).  Three rows in ten are fathers (two in a hundred of a large cloud, to keep the output small)."""
    g = torch.Generator().manual_seed(seed + 13 * P + K)
    B = len(lens)
    pts = torch.rand(B, P, 3, generator=g) * 2 - 1
    knn = torch.stack([torch.randint(0, max(l, 1), (P, K), generator=g) for l in lens])
    knn[:, ::5, K - 3:] = -1
    knn[:, 2::9] = -1
    knn[:, 1::4, :K - patch] = -1                       # (the columns a wider list has in front: never read)
    father = (torch.rand(B, P, generator=g) < (0.3 if P < 100000 else 0.02)) & (torch.arange(P)[None, :] < torch.tensor(lens)[:, None])
    rank = father.long().cumsum(dim=1)
    per = rank[:, -1] * patch
    first = per.cumsum(0) - per + 3 * (torch.arange(B) + 1)
    return pts, knn, father.to(torch.uint8), rank, first, int(per.sum()) + 3 * B + 3


# (P, lens, K)
CHILDREN_CASES = [(P, [P], K) for P in (1, 255, 257) for K in (8, 16)] + [(1000, [1000, 700, 0], 8), (1000, [1000, 700, 0], 16),
                                                                          (SECOND_SWEEP_256, [SECOND_SWEEP_256], 8)]


def insert_inputs(P=1000, lens=(1000, 700, 0), R=400, seed=5):
    """The B = 3 batch of the end-to-end insert test: jittered unit-sphere clouds (zero rows past each length), a
    reference cloud of R sphere points and a heavy-tailed metric."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    points = torch.stack([unit(P) + 0.02 * (torch.rand(P, 3, generator=g) - 0.5) for _ in lens])
    for b, l in enumerate(lens):
        points[b, l:] = 0
    return unit(R), torch.exp(3 * torch.randn(R, 1, generator=g)), points, torch.tensor(lens, dtype=torch.int64)


def insert(ref_points, ref_metrics, points, lens, search):
    """UniformProjection.insert (levelset_sampling.py:172-233) on a padded batch, fathers and children in float64.
    `search(points, points, lens, lens, K, r)` -> (d2, idx, ...) is the neighbour search (not one of the five
    operations: the CPU oracle's).  Returns dict(selected, spacing, radius, father, fenced, children [per cloud],
    sizes)."""
    B, P = points.shape[:2]
    R = ref_points.shape[0]
    flat = points.reshape(-1, 3).double()
    diag = float((flat.max(dim=0).values - flat.min(dim=0).values).norm())
    spacing = math.sqrt(diag / R)
    patch = 8
    radius = min(spacing * patch, 0.2)
    _, idx, _, _ = search(points, points, lens, lens, K=patch + 1, r=radius)
    metric = ref_metrics.reshape(-1)
    bar = min(metric.median() * 2, metric.max() * 0.5)
    sel = ref_points[metric > bar]
    cap = min(50, R // 20)
    if sel.shape[0] == 0 or sel.shape[0] > cap:
        sel = ref_points[metric.sort(dim=0).indices[-max(cap, 1):]]
    params = torch.tensor([(4 * radius) ** 2, 4 * spacing ** 2], dtype=torch.float32)
    mask, _, fenced = fathers(points, lens, sel, sel.shape[0], params)
    per = mask.sum(dim=1) * patch
    first = per.cumsum(0) - per
    packed = children(points, idx[..., 1:], mask, first, patch, int(per.sum()))
    kids = [packed[int(first[b]):int(first[b] + per[b])] for b in range(B)]
    return dict(selected=sel, spacing=spacing, radius=radius, father=mask, fenced=fenced, children=kids,
                sizes=[int(v) for v in per])
