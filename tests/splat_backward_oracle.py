"""Float64 reference of the splat backward pass (iso_points_amd/csrc/splat_backward.hip) -- numpy on the CPU, test
infrastructure only -- and the inputs of the cases test_splat_backward_cpu.py / test_splat_backward_gpu.py share.

occ_backward64      xy gradient of the occupancy image.  Rules: rasterize_points_backward.cu:156-161 (disc support),
                    rasterize_points.cu:726-746 (rectangle support) and `occ_term` in the kernel file; pixel centres
                    follow splat_frame.h (the short side spans [-1, 1], a pixel is 2 / min(H, W) wide, both axes
                    flipped: output column xo holds NDC index W - 1 - xo).
zbuf_backward_exact the exactly rounded z sum (ZbufBackwardKernel, rasterize_points.cu:823-846).
visible_and_radius  visible set and search radius of EllipticalRasterizer.backward (rasterizer.py:850-884).
path_census         which branch of the kernels each point and each 8x8 block takes, from the integers alone.

The bound the GPU result is held to, per point and component (occ_bound):

    |got - ref64| <= (n_terms + 8) * 2^-24 * abs_sum + unc_sum

A float32 term dx / denom * g carries seven relative roundings of 2^-24 to first order: dx (one); dist2 = fl(fl(dx dx)
+ fl(dy dy)) inherits 2 from dx or dy, one from the product and one from the sum (four, all terms positive); the quotient
adds one to dx's and dist2's (six), the product with g one more (seven) -- eight leaves one for the second-order terms.
A lane adds its terms in image order starting from 0 (the first addition is exact) and the eight lane sums meet in a
three-level tree that rounds only where both operands are non-zero: a term passes through at most n_terms - 1 rounded
additions, each of a partial sum bounded by abs_sum.  unc_sum covers the pixels whose membership the float32 kernel
may decide differently: the terms of every pixel with a membership test within a relative 2^-20 (eight float32 ulps:
three or four roundings between inputs and comparison) of its threshold, unless every quantity that enters that
comparison is a float32 number (then float32 and float64 compute the same values and decide alike).
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

F32 = np.float32
F64 = np.float64
MARGIN = 2.0 ** -20
EPS = float(F32(1e-10))
GB = 8                     # pixels per block side; 8 x 8 blocks per super block
RY = 4                     # block rows per round of the heavy kernel
HEAVY_STRIDE = 4096 * 32   # heavy points per stride of the heavy kernel (workgroups x points per workgroup)


def _np(t, dt):
    if t is None:
        return None
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=dt)


Frame = namedtuple("Frame", "H W m ex ey xs ys")


def frame(H, W):
    """splat_frame.h in float32: half extents and the centre of every OUTPUT column / row (axes flipped)."""
    m = min(H, W)
    ex, ey = F32(W) / F32(m), F32(H) / F32(m)
    ix = np.arange(W - 1, -1, -1)
    iy = np.arange(H - 1, -1, -1)
    xs = -ex + ((2 * ix).astype(F32) + F32(1.0)) / F32(m)
    ys = -ey + ((2 * iy).astype(F32) + F32(1.0)) / F32(m)
    assert xs.dtype == F32 and ys.dtype == F32
    return Frame(H, W, m, ex, ey, xs, ys)


def _rep(x):
    """x (float64) is a float32 number"""
    with np.errstate(over="ignore"):
        return x.astype(F32).astype(F64) == x


def _near(a, t):
    return np.abs(a - t) <= MARGIN * np.abs(t)


Terms = namedtuple("Terms", "tx ty inc unc tie zero")


def _terms(g, dx, dy, rx, ry, sx, sy, r, rect, out_exact):
    """All float64, broadcastable.  g: gradient of the pixel, (dx, dy): centre - point, (rx, ry): ellipse box, (sx, sy):
    rectangle support, r: disc radius, out_exact: the kernel's box half widths equal rx, ry exactly.
    -> the two terms of every pixel, which pixels the sum includes, which are uncertain, which sit exactly on a
    threshold and which have dist2 = 0."""
    adx, ady = np.abs(dx), np.abs(dy)
    dist2 = dx * dx + dy * dy
    has = g != 0.0
    if rect:
        inside = (adx <= sx) & (ady <= sy)
        near_in = (_near(adx, sx) & ~(_rep(dx) & _rep(sx))) | (_near(ady, sy) & ~(_rep(dy) & _rep(sy)))
        tie = (adx == sx) | (ady == sy)
    else:
        r2 = r * r
        inside = dist2 <= r2
        exact = _rep(dx) & _rep(dy) & _rep(dx * dx) & _rep(dy * dy) & _rep(dist2) & _rep(r2)
        near_in = _near(dist2, r2) & ~exact
        tie = dist2 == r2
    outside = (adx > rx) | (ady > ry)
    near_out = (_near(adx, rx) & ~(_rep(dx) & out_exact)) | (_near(ady, ry) & ~(_rep(dy) & out_exact))
    tie = tie | (inside & ((adx == rx) | (ady == ry)))
    inc = has & inside & ~((g > 0.0) & outside)
    unc = has & (near_in | ((inside | near_in) & (g > 0.0) & near_out))
    denom = np.maximum(dist2, EPS)               # sign-preserving eps denominator; dist2 >= 0
    return Terms(dx / denom * g, dy / denom * g, inc, unc, has & tie, has & inside & (dist2 == 0.0))


OccRef = namedtuple("OccRef", "grad n_terms abs_sum unc_sum n_unc n_tie n_zero_dist")


def _setup(points, radii, grad_occ, first, num, rs, visible, rect, radii_s):
    pts, ra, go = _np(points, F32), _np(radii, F32), _np(grad_occ, F32)
    fi, nu = _np(first, np.int64), _np(num, np.int64)
    N, H, W = go.shape
    P = pts.shape[0]
    fr = frame(H, W)
    cloud = np.full(P, -1, np.int64)
    for n in range(N):
        cloud[fi[n]:fi[n] + nu[n]] = n
    cl = np.maximum(cloud, 0)
    s32 = F32(radii_s)
    if rect:
        sx32, sy32 = ra[:, 0] * s32, ra[:, 1] * s32                # the float32 products the kernel forms
        sx, sy = ra[:, 0].astype(F64) * float(s32), ra[:, 1].astype(F64) * float(s32)
        r = np.zeros(P)
        out_exact = _rep(sx) & _rep(sy) & ((sx32 / s32) == ra[:, 0]) & ((sy32 / s32) == ra[:, 1])
    else:
        r32 = _np(rs, F32)[cl]
        sx32 = sy32 = r32
        sx = sy = r = r32.astype(F64)
        out_exact = np.ones(P, bool)
    vis = np.ones(P, bool) if visible is None else _np(visible, np.uint8) != 0
    px, py, pz = pts[:, 0], pts[:, 1], pts[:, 2]
    live = (cloud >= 0) & vis & ~((pz < 0) | (np.abs(py) > fr.ey) | (np.abs(px) > fr.ex)) & (sx32 > 0) & (sy32 > 0)
    return dict(pts=pts, ra=ra, go=go, fr=fr, cloud=cloud, cl=cl, sx32=sx32, sy32=sy32, sx=sx, sy=sy, r=r,
                out_exact=out_exact, live=live, N=N, H=H, W=W, P=P, fi=fi, nu=nu)


def _empty(P):
    return OccRef(np.zeros((P, 2)), np.zeros(P, np.int64), np.zeros((P, 2)), np.zeros((P, 2)), np.zeros(P, np.int64),
                  np.zeros(P, np.int64), np.zeros(P, np.int64))


def _window(c, s, n, e, m):
    """float64 bound of the OUTPUT pixels of an axis whose centre may lie within c +- s, widened by two pixels"""
    lo = np.floor(((c - s) + e) * 0.5 * m - 0.5) - 2
    hi = np.ceil(((c + s) + e) * 0.5 * m - 0.5) + 2
    lo = np.clip(lo, 0, n - 1).astype(np.int64)
    hi = np.clip(hi, 0, n - 1).astype(np.int64)
    return n - 1 - hi, n - 1 - lo


def occ_backward64(points, radii, grad_occ, first, num, *, rs=None, visible=None, rect=False, radii_s=10.0):
    """xy gradient of the occupancy image in float64 from the float32 inputs and pixel centres the kernel sees; every
    point visits the pixel window of its support only.  -> OccRef: grad (P,2), n_terms (P,), abs_sum (P,2) = sum |term|,
    unc_sum (P,2) = sum |term| over the uncertain pixels (module docstring), and three pixel counts per point:
    uncertain, exactly on a threshold, at distance 0."""
    S = _setup(points, radii, grad_occ, first, num, rs, visible, rect, radii_s)
    fr, P = S["fr"], S["P"]
    out = _empty(P)
    ids = np.nonzero(S["live"])[0]
    if ids.size == 0:
        return out
    px, py = S["pts"][ids, 0].astype(F64), S["pts"][ids, 1].astype(F64)
    x0, x1 = _window(px, S["sx"][ids], fr.W, float(fr.ex), fr.m)
    y0, y1 = _window(py, S["sy"][ids], fr.H, float(fr.ey), fr.m)
    area = (x1 - x0 + 1) * (y1 - y0 + 1)
    order = np.argsort(area, kind="stable")
    xs64, ys64, go = fr.xs.astype(F64), fr.ys.astype(F64), S["go"]
    budget = 1 << 20
    i = 0
    while i < order.size:
        # points of similar window size share a padded (points, rows, columns) batch
        j = i + 1
        hh, ww = y1[order[i]] - y0[order[i]] + 1, x1[order[i]] - x0[order[i]] + 1
        while j < order.size:
            h2 = max(hh, y1[order[j]] - y0[order[j]] + 1)
            w2 = max(ww, x1[order[j]] - x0[order[j]] + 1)
            if (j + 1 - i) * h2 * w2 > budget:
                break
            hh, ww, j = h2, w2, j + 1
        sel = order[i:j]
        p = ids[sel]
        yy = y0[sel, None] + np.arange(hh)[None, :]
        xx = x0[sel, None] + np.arange(ww)[None, :]
        vy, vx = yy <= y1[sel, None], xx <= x1[sel, None]
        yy, xx = np.minimum(yy, fr.H - 1), np.minimum(xx, fr.W - 1)
        g = go[S["cl"][p][:, None, None], yy[:, :, None], xx[:, None, :]].astype(F64)
        g = np.where(vy[:, :, None] & vx[:, None, :], g, 0.0)
        col = lambda a: a[p].astype(F64)[:, None, None]
        T = _terms(g, xs64[xx][:, None, :] - px[sel, None, None], ys64[yy][:, :, None] - py[sel, None, None],
                   col(S["ra"][:, 0]), col(S["ra"][:, 1]), col(S["sx"]), col(S["sy"]), col(S["r"]), rect,
                   S["out_exact"][p][:, None, None])
        _reduce(out, p, T)
        i = j
    return out


def _reduce(out, p, T):
    ax = tuple(range(1, T.tx.ndim))
    for c, t in enumerate((T.tx, T.ty)):
        out.grad[p, c] = np.where(T.inc, t, 0.0).sum(axis=ax)
        out.abs_sum[p, c] = np.where(T.inc, np.abs(t), 0.0).sum(axis=ax)
        out.unc_sum[p, c] = np.where(T.unc, np.abs(t), 0.0).sum(axis=ax)
    out.n_terms[p] = T.inc.sum(axis=ax)
    out.n_unc[p] = T.unc.sum(axis=ax)
    out.n_tie[p] = T.tie.sum(axis=ax)
    out.n_zero_dist[p] = T.zero.sum(axis=ax)


def occ_backward64_full(points, radii, grad_occ, first, num, *, rs=None, visible=None, rect=False, radii_s=10.0):
    """The same formulas over every pixel of the point's image, one point at a time (small cases only)."""
    S = _setup(points, radii, grad_occ, first, num, rs, visible, rect, radii_s)
    fr = S["fr"]
    out = _empty(S["P"])
    xs64, ys64 = fr.xs.astype(F64)[None, None, :], fr.ys.astype(F64)[None, :, None]
    for p in np.nonzero(S["live"])[0]:
        T = _terms(S["go"][S["cl"][p]].astype(F64)[None], xs64 - float(S["pts"][p, 0]), ys64 - float(S["pts"][p, 1]),
                   float(S["ra"][p, 0]), float(S["ra"][p, 1]), S["sx"][p], S["sy"][p], S["r"][p], rect,
                   S["out_exact"][p])
        _reduce(out, np.array([p]), T)
    return out


def occ_bound(ref):
    """(P,2): the bound of the module docstring"""
    return (ref.n_terms[:, None] + 8) * 2.0 ** -24 * ref.abs_sum + ref.unc_sum


# --------------------------------------------------------------------------------------------------- z gradient
def zbuf_backward_exact(idx, grad_zbuf, P):
    """-> (exact (P,) float64: the correctly rounded sum per point of grad_zbuf over the slots that list it, NaN where
    one of them is NaN or Inf; n_p (P,): the number of such slots).  Zeros are skipped, a pixel's list ends at the
    first idx < 0."""
    ii, gz = _np(idx, np.int32), _np(grad_zbuf, F32)
    K = ii.shape[-1]
    ii, gz = ii.reshape(-1, K), gz.reshape(-1, K)
    valid = (np.cumprod(ii >= 0, axis=1) != 0) & (gz != 0.0)
    p, v = ii[valid].astype(np.int64), gz[valid].astype(F64)
    assert p.size == 0 or p.max() < P
    order = np.argsort(p, kind="stable")
    p, v = p[order], v[order]
    n_p = np.bincount(p, minlength=P).astype(np.int64)
    ends = np.cumsum(n_p)
    exact = np.zeros(P)
    for q in np.nonzero(n_p)[0]:
        t = v[ends[q] - n_p[q]:ends[q]]
        exact[q] = math.fsum(t.tolist()) if np.isfinite(t).all() else float("nan")
    return exact, n_p


def z_quantum(grad_zbuf, pixels_per_view):
    """q = 2^-(61 - terms_log2 - ex), ex from frexp(max |g|): the fixed-point step the comment above k_z_scatter
    promises (0 when every g is 0).  The maximum is the largest FINITE magnitude: a NaN or an Inf poisons the points
    that receive it and must cost the others nothing."""
    gz = _np(grad_zbuf, F32)
    a = np.abs(gz[np.isfinite(gz)])
    mx = float(a.max()) if a.size else 0.0
    if mx == 0.0:
        return 0.0
    terms_log2 = int(math.ceil(math.log2(pixels_per_view)))
    ex = math.frexp(mx)[1]
    return 2.0 ** -(61 - terms_log2 - ex)


def z_bound(exact, n_p, q):
    return n_p * (q / 2) + (2.0 ** -24 + 2.0 ** -50) * np.abs(exact)


def synthetic_lists(N, H, W, K, P, seed):
    """(N,H,W,K) int32 lists for the z tests: random points, a random -1 suffix per pixel (whole pixels empty too),
    and three points that head the lists of thousands of pixels."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, P, (N, H, W, K), generator=g, dtype=torch.int32)
    lens = torch.randint(0, K + 1, (N, H, W), generator=g)
    hot = (torch.rand(N, H, W, generator=g) < 0.3) & (lens > 0)
    idx[..., 0][hot] = torch.randint(0, 3, (int(hot.sum()),), generator=g, dtype=torch.int32) * (P // 3)
    idx[torch.arange(K)[None, None, None, :] >= lens[..., None]] = -1
    return idx.contiguous()


# --------------------------------------------------------------------------------------------------- visible set
def visible_and_radius(idx, radii, first, num, radii_s):
    """rasterizer.py:850-884 -> (visible (P,) bool: the points listed in a pixel whose first slot is filled;
    rs (N,) float32: the lower median of both radius columns of the cloud's visible points, times radii_s)."""
    ii, ra = _np(idx, np.int32), _np(radii, F32)
    fi, nu = _np(first, np.int64), _np(num, np.int64)
    K = ii.shape[-1]
    ii = ii.reshape(-1, K)
    listed = ii[ii[:, 0] >= 0].reshape(-1)
    vis = np.zeros(ra.shape[0], bool)
    vis[listed[listed >= 0]] = True
    rs = np.zeros(len(fi), F32)
    for n in range(len(fi)):
        rv = np.sort(ra[fi[n]:fi[n] + nu[n]][vis[fi[n]:fi[n] + nu[n]]].reshape(-1))
        if rv.size:
            rs[n] = rv[(rv.size - 1) // 2] * F32(radii_s)
    return vis, rs


# --------------------------------------------------------------------------------------------------- path census
def _pixel_range(c, r, n, e, m):
    """pixel_range + out_range of the kernel files in float32 -> (ok, lo, hi) in output pixels"""
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (r >= 0) & (c == c)
        flo = ((c - r) + e) * F32(0.5) * F32(m) - F32(0.5)
        fhi = ((c + r) + e) * F32(0.5) * F32(m) - F32(0.5)
        assert flo.dtype == F32
        ok &= (flo < F32(1e9)) & (fhi > F32(-1e9))
        flo = np.where(ok, np.maximum(flo, F32(-4.0)), F32(0))
        fhi = np.where(ok, np.minimum(fhi, F32(n) + F32(4.0)), F32(0))
    lo = np.maximum(np.ceil(flo).astype(np.int64) - 1, 0)
    hi = np.minimum(np.floor(fhi).astype(np.int64) + 1, n - 1)
    ok &= lo <= hi
    return ok, n - 1 - hi, n - 1 - lo


CENSUS_KEYS = ("skipped", "light_zero", "heavy", "heavy_strides", "word_rounds_gt1", "row_rounds_gt1", "dense_blocks",
               "scan_blocks", "clip_left", "clip_right", "clip_top", "clip_bottom", "last_word_reads", "nb2x", "nb2y")


def path_census(points, radii, rs, grad_occ, first, num, rect=False, radii_s=10.0, visible=None, aligned=True,
                blocks=True):
    """Which branch each point and each 8x8 block takes, from the pixel_range block ranges of splat_frame.h and the
    8x8 / 64x64 maps of the gradient image.  Counts of points: skipped (invisible, z < 0, off frame, no support),
    light_zero (support touches no flagged super block), heavy, word_rounds_gt1 (heavy, more than one `cx` round),
    row_rounds_gt1 (heavy, more than RY block rows), last_word_reads (heavy, last cloud, window reaching the last block
    row, a round at cx = NB2x - 1); heavy_strides = strides of the heavy kernel's loop.  Counts of (heavy point,
    flagged block) pairs (blocks=True): dense_blocks (row path), scan_blocks (bit scans), clip_* (the window cuts the
    block on that side).  aligned: the image base pointer is 16-byte aligned."""
    S = _setup(points, radii, grad_occ, first, num, rs, visible, rect, radii_s)
    fr, N, H, W = S["fr"], S["N"], S["H"], S["W"]
    NBx, NBy = (W + GB - 1) // GB, (H + GB - 1) // GB
    NB2x, NB2y = (NBx + 7) // 8, (NBy + 7) // 8
    nz = np.zeros((N, NBy * GB, NBx * GB), bool)
    nz[:, :H, :W] = S["go"] != 0
    pix = nz.reshape(N, NBy, GB, NBx, GB).transpose(0, 1, 3, 2, 4)        # (N, NBy, NBx, 8, 8)
    flag = pix.any(axis=(3, 4))
    f2 = np.zeros((N, NB2y * 8, NB2x * 8), bool)
    f2[:, :NBy, :NBx] = flag
    blk2 = f2.reshape(N, NB2y, 8, NB2x, 8).any(axis=(2, 4))
    c = dict.fromkeys(CENSUS_KEYS, 0)
    c["nb2x"], c["nb2y"] = NB2x, NB2y
    in_cloud = S["cloud"] >= 0
    okx, x0, x1 = _pixel_range(S["pts"][:, 0], S["sx32"], W, fr.ex, fr.m)
    oky, y0, y1 = _pixel_range(S["pts"][:, 1], S["sy32"], H, fr.ey, fr.m)
    cand = S["live"] & okx & oky
    c["skipped"] = int((in_cloud & ~cand).sum())
    # image order of the census does not matter: counts only
    row0 = np.arange(GB)
    for p in np.nonzero(cand)[0]:
        n = S["cl"][p]
        if not blk2[n, y0[p] // 64:y1[p] // 64 + 1, x0[p] // 64:x1[p] // 64 + 1].any():
            c["light_zero"] += 1
            continue
        c["heavy"] += 1
        bx0, bx1, by0, by1 = x0[p] // GB, x1[p] // GB, y0[p] // GB, y1[p] // GB
        cxs = range(bx0 >> 3, (bx1 >> 3) + 1, 4)
        c["word_rounds_gt1"] += len(cxs) > 1
        c["row_rounds_gt1"] += (by1 - by0) >= RY
        c["last_word_reads"] += bool(n == N - 1 and by1 == NBy - 1 and (NB2x - 1) in cxs)
        if not blocks:
            continue
        bys, bxs = np.arange(by0, by1 + 1), np.arange(bx0, bx1 + 1)
        rows = bys[:, None] * GB + row0[None, :]
        cols = bxs[:, None] * GB + row0[None, :]
        rsel = (rows >= y0[p]) & (rows <= y1[p])                               # (hb, 8)
        csel = (cols >= x0[p]) & (cols <= x1[p])                               # (wb, 8)
        win = rsel[:, None, :, None] & csel[None, :, None, :]                  # (hb, wb, 8, 8)
        sub = pix[n, by0:by1 + 1, bx0:bx1 + 1]
        fl = flag[n, by0:by1 + 1, bx0:bx1 + 1]
        m = sub & win
        whole = (m == win).all(axis=(2, 3))
        fits = ((bxs * GB + GB) <= W)[None, :] & (W % 4 == 0) & bool(aligned)
        dense = fl & whole & fits
        c["dense_blocks"] += int(dense.sum())
        c["scan_blocks"] += int((fl & ~dense & m.any(axis=(2, 3))).sum())
        c["clip_top"] += int((fl & ~rsel[:, 0][:, None]).sum())
        c["clip_bottom"] += int((fl & ~rsel[:, GB - 1][:, None]).sum())
        c["clip_left"] += int((fl & ~csel[:, 0][None, :]).sum())
        c["clip_right"] += int((fl & ~csel[:, GB - 1][None, :]).sum())
    c["heavy_strides"] = (c["heavy"] + 63) // 64 * 64 // HEAVY_STRIDE + ((c["heavy"] + 63) // 64 * 64 % HEAVY_STRIDE > 0)
    return {k: int(v) for k, v in c.items()}


# --------------------------------------------------------------------------------------------------- the cases
def _rand_points(g, P, H, W, spread=1.05, hidden=0.2, zneg=0.1, zero_r=0.05):
    """random points spread beyond the frame, some z < 0, some zero radii, ellipse radii rx != ry in [0.01, 0.12] and a
    `visible` mask that hides a share of them"""
    m = min(H, W)
    ext = torch.tensor([W / m, H / m]) * spread
    pts = torch.cat([(torch.rand(P, 2, generator=g) * 2 - 1) * ext, torch.rand(P, 1, generator=g) * 3 + 0.1], dim=1)
    pts[torch.rand(P, generator=g) < zneg, 2] = -0.5
    radii = 0.01 + 0.11 * torch.rand(P, 2, generator=g)
    radii[torch.rand(P, generator=g) < zero_r] = 0.0
    visible = (torch.rand(P, generator=g) >= hidden).to(torch.uint8)
    return pts.contiguous(), radii.contiguous(), visible


def _grad(g, N, H, W, density):
    go = torch.randn(N, H, W, generator=g)                     # mixed signs
    if density < 1.0:
        go[torch.rand(N, H, W, generator=g) >= density] = 0.0
    return go


def _split(P, N):
    num = torch.tensor([P // N] * (N - 1) + [P - (P // N) * (N - 1)])
    return torch.cumsum(num, 0) - num, num


def _case_g(rect):
    """64 points on the centres of the pixels (8 i + 4, 8 j + 4) of a 64 x 64 image, gradients on single pixels: the
    same lattice (distance 0 to its own point: the eps denominator; 8 px = 0.25 to the neighbours': exactly on the disc
    rim, on the box edge of the points with rx = 0.25, and on the rectangle edge of those with rx * radii_s = 0.25)
    and pixels 3 px right, 4 px up of every second lattice site (inside the disc, outside the small boxes: kept for
    g < 0, dropped for g > 0).  Every value is a small multiple of 1/32: every decision is exact in float32."""
    fr = frame(64, 64)
    go = torch.zeros(1, 64, 64)
    pts = torch.zeros(64, 3)
    radii = torch.zeros(64, 2)
    for i in range(8):
        for j in range(8):
            k = 8 * i + j
            yo, xo = 8 * i + 4, 8 * j + 4
            pts[k] = torch.tensor([float(fr.xs[xo]), float(fr.ys[yo]), 1.0])
            sign = 1.0 if (i + j // 2) % 2 == 0 else -1.0
            go[0, yo, xo] = sign * (1.0 + k / 8.0)
            if k % 2 == 0:
                go[0, yo - 4, xo + 3] = -sign * (0.5 + k / 16.0)
            if rect:       # radii_s = 4: supports of 4, 8 and 32 px
                radii[k] = torch.tensor([(1.0, 2.0, 8.0)[k % 3] / 32.0, (2.0, 1.0, 8.0)[(k // 3) % 3] / 32.0])
            else:          # boxes of 2, 8 and 16 px
                radii[k] = torch.tensor([(2.0, 8.0, 16.0)[k % 3] / 32.0, (8.0, 2.0, 16.0)[(k // 3) % 3] / 32.0])
    first, num = _split(64, 1)
    return dict(points=pts, radii=radii, visible=None, go=go, first=first, num=num,
                rs=None if rect else torch.tensor([0.25]), rect=rect, radii_s=4.0 if rect else 10.0)


# name -> (H, W, clouds, points, gradient, support).  What each is there for: test_splat_backward_cpu.REACHES
CASES = ("a", "b", "c_sparse", "c_dense", "d1_sparse", "d2_dense", "e", "f_dense", "f_ring", "g_disc", "g_rect", "h")


@lru_cache(maxsize=None)
def case(name):
    """The inputs of a case (CPU tensors; treat as read-only): points, radii, visible, go (N,H,W), first, num, rs,
    rect, radii_s."""
    g = torch.Generator().manual_seed(1000 + CASES.index(name))
    rect, radii_s, rs = False, 10.0, None
    if name in ("g_disc", "g_rect"):
        return _case_g(name == "g_rect")
    if name in ("a", "b"):
        H, W, N, P = 72, 72, 2, 600
        go = _grad(g, N, H, W, 0.02 if name == "a" else 1.0)
        rs = torch.tensor([0.35, 0.2])
    elif name in ("c_sparse", "c_dense"):
        H, W, N, P = 130, 67, 2, 600
        go = _grad(g, N, H, W, 0.05 if name == "c_sparse" else 1.0)
        rs = torch.tensor([0.5, 0.5])
    elif name in ("d1_sparse", "d2_dense"):
        H, W, P = 72, 328, 400
        N = 1 if name == "d1_sparse" else 2
        go = _grad(g, N, H, W, 0.02 if name == "d1_sparse" else 1.0)
        # a pixel is 1/36 wide: a disc of 1.6 spans 16 blocks, one of 4.0 spans 37 (a second word round needs > 32)
        rs = torch.tensor([4.0] if N == 1 else [1.6, 4.0])
    elif name == "e":
        H, W, N, P = 200, 136, 2, 500
        go = torch.zeros(N, H, W)                      # one 64 x 64 super block per cloud holds all of the gradient
        go[0, 64:128, 64:128] = _grad(g, 1, 64, 64, 0.2)[0]
        go[1, 128:192, 0:64] = _grad(g, 1, 64, 64, 0.2)[0]
        rs = torch.tensor([0.3, 0.3])
    elif name in ("f_dense", "f_ring"):
        H, W, N, P = 136, 200, 2, 500
        go = _grad(g, N, H, W, 1.0)
        rect = True
        radii_s = 6.0 if name == "f_dense" else 10.0
        if name == "f_ring":
            yy, xx = torch.meshgrid(torch.arange(H) - 67.5, torch.arange(W) - 99.5, indexing="ij")
            d = torch.sqrt(yy * yy + xx * xx)
            go[:, (d < 40) | (d > 52)] = 0.0
    elif name == "h":
        # heavy list > 131 072 of 140 001 points: nearly every point has to be visible, in front and on the frame
        H, W, N = 72, 72, 3
        num = torch.tensor([0, 1, 140000])
        pts, radii, visible = _rand_points(g, 140001, H, W, spread=1.005, hidden=0.01, zneg=0.01)
        return dict(points=pts, radii=radii, visible=visible, go=_grad(g, N, H, W, 0.3), first=torch.cumsum(num, 0) - num,
                    num=num, rs=torch.tensor([0.05, 0.05, 0.05]), rect=False, radii_s=10.0)
    else:
        raise KeyError(name)
    pts, radii, visible = _rand_points(g, P, H, W)
    first, num = _split(P, N)
    return dict(points=pts, radii=radii, visible=visible, go=go, first=first, num=num, rs=rs, rect=rect, radii_s=radii_s)


@lru_cache(maxsize=None)
def case_ref(name):
    c = case(name)
    return occ_backward64(c["points"], c["radii"], c["go"], c["first"], c["num"], rs=c["rs"], visible=c["visible"],
                          rect=c["rect"], radii_s=c["radii_s"])


@lru_cache(maxsize=None)
def case_census(name, aligned=True):
    c = case(name)
    return path_census(c["points"], c["radii"], c["rs"], c["go"], c["first"], c["num"], rect=c["rect"],
                       radii_s=c["radii_s"], visible=c["visible"], aligned=aligned, blocks=name != "h")
