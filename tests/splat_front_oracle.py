"""Plain references of stage 1 of the splat pipeline (csrc/splat.hip): the renderable test, the packed layout, the
per-point EWA set-up, the gradient of the packed NDC rows to the world points and the isotropic bandwidth.  Plain
torch on the CPU, no HIP.

Two precisions of each arithmetic statement:
  * float64: the truth an error is measured against (mask64, setup64, points_backward64);
  * float32 with the kernel's own statements and association (flags_ref, setup32, points_backward32): every
    operation below is ONE torch elementwise op on float32 tensors, i.e. one correctly rounded IEEE operation without
    contraction, as the kernels are built (-ffp-contract=off, correctly rounded division and square root).  setup32 is
    the yardstick of the accuracy rule  e_hip <= 1.5 e_setup32 + 2e-7;  flags_ref is what an exact match is asserted
    against.

What the bit-for-bit assertions against setup32 / points_backward32 rest on (test_splat_front_gpu.py: the helper axis
on ties, the zero frame): the host's torch evaluates every float32 elementwise multiply, add, subtract and divide as
one IEEE operation, and the square root is taken through float64 (_sqrt: torch's own float32 sqrt on a CPU is not
correctly rounded).  A torch build that fused multiply-add inside a CPU elementwise chain would show up in those
tests as a kernel failure though the kernel had not changed: check this module first.
"""
import math

import torch

from oracle import splat_oracle as SO

F32, F64 = torch.float32, torch.float64
CHUNK = 1024                      # points per workgroup of the front end (kChunk)


# ----------------------------------------------------------------------------- renderable test
def _zdot(p, V, dtype, affine):
    """((x V[0][2] + y V[1][2]) + z V[2][2]) (+ V[3][2]): the kernel's association, one rounding per operation."""
    p, V = p.to(dtype), V.to(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = (x * V[0, 2] + y * V[1, 2]) + z * V[2, 2]
    return r + V[3, 2] if affine else r


def flags_ref(points, normals, views, znear=1.0, zfar=100.0, backface=True, dtype=F32):
    """(N, P) bool: znear <= z_view <= zfar (both inclusive) and, with backface culling, (view-space normal).z < 0
    (strict) -- the reference's filter_renderable, rasterizer.py:184-254, in the kernel's float32 association."""
    out = []
    for V in views:
        zv = _zdot(points, V, dtype, True)
        ok = (zv >= znear) & (zv <= zfar)
        if backface:
            ok = ok & (_zdot(normals, V, dtype, False) < 0)
        out.append(ok)
    return torch.stack(out) if out else torch.zeros((0, points.shape[0]), dtype=torch.bool)


def mask64(points, normals, views, znear=1.0, zfar=100.0, backface=True):
    """The same test in float64 (the thresholds compare exactly where the inputs are exactly representable)."""
    return flags_ref(points, normals, views, znear, zfar, backface, dtype=F64)


def mask_bits(flags):
    """(N, P) bool -> (P,) int32, bit v = renderable in view v."""
    n = flags.shape[0]
    w = (1 << torch.arange(n, dtype=torch.int64))[:, None]
    return (flags.to(torch.int64) * w).sum(0).to(torch.int32)


def bits_to_flags(mask, n_views):
    return ((mask.to(torch.int64)[None, :] >> torch.arange(n_views, dtype=torch.int64)[:, None]) & 1).bool()


def pack_ref(mask, n_views):
    """first_idx (N,) i64, num_points (N,) i64, src (T,) i32 of the packed layout (view-major, points ascending:
    rasterizer.py:597-618) by plain boolean indexing.  mask: (P,) int bit mask or (N, P) bool."""
    flags = mask if mask.dtype == torch.bool else bits_to_flags(mask, n_views)
    ar = torch.arange(flags.shape[1], dtype=torch.int32)
    src = [ar[flags[v]] for v in range(n_views)]
    num = torch.tensor([s.numel() for s in src], dtype=torch.int64)
    first = torch.cumsum(num, 0) - num
    return first, num, (torch.cat(src) if src else ar[:0])


def view_total_ref(num):
    vt = torch.zeros(8, dtype=torch.int32)
    vt[:num.numel()] = num.to(torch.int32)
    return vt


# ----------------------------------------------------------------------------- per-point EWA set-up
def _sqrt(x):
    """A correctly rounded square root in the precision of x, as the kernels' sqrtf is: torch's float32 sqrt on a CPU is
    not (it differs in the last place on up to a fifth of its arguments, depending on the host), and the root of the
    double is, rounded once more (53 >= 2 * 24 + 2 bits: the second rounding is innocuous)."""
    return torch.sqrt(x.double()).to(x.dtype) if x.dtype == F32 else torch.sqrt(x)


def _eps_denom(x, eps=1e-17):
    s = torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x))
    return s * x.abs().clamp(min=eps)


def _frame(n):
    """splat_setup_point's tangent frame, statement by statement: e = the axis least aligned with n (x before y before
    z on ties), u = normalize(n x (n + e)), v = normalize(n x u), norms clamped at 1e-12."""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    ax, ay, az = nx.abs(), ny.abs(), nz.abs()
    is_x = (ax <= ay) & (ax <= az)
    is_y = ~is_x & (ay <= az)
    is_z = ~is_x & ~is_y
    one = lambda b: b.to(n.dtype)                                           # noqa: E731
    mx, my, mz = nx + one(is_x), ny + one(is_y), nz + one(is_z)

    def cross_unit(bx, by, bz):
        cx, cy, cz = ny * bz - nz * by, nz * bx - nx * bz, nx * by - ny * bx
        norm = _sqrt((cx * cx + cy * cy) + cz * cz).clamp(min=1e-12)
        return cx / norm, cy / norm, cz / norm

    u = cross_unit(mx, my, mz)
    return u, cross_unit(*u)


def _setup_kernel_form(points, normals, h, V, M, S, sigma, cutoff, dtype, radii_form, frame=None):
    """The statements of splat_setup_point (csrc/splat.hip) in `dtype`, one torch op per kernel operation.
    radii_form: "den" = sqrt(4 a cutoff / (4ac - b^2)) (the reference's statement), "g" = sqrt(g00 cutoff),
    sqrt(g11 cutoff) (equal in exact arithmetic: 4ac - b^2 = 4 / det G).  frame: (2, P, 3) u, v to use instead of
    the kernel's own (any orthonormal basis of the tangent plane gives the same result in exact arithmetic)."""
    c = lambda t: t.to(dtype)                                               # noqa: E731
    p, n, hk, V, M = c(points), c(normals), c(h), c(V), c(M)
    k = lambda v: torch.tensor(v, dtype=dtype)                              # noqa: E731  (a scalar of the working precision)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    xv = ((x * M[0, 0] + y * M[1, 0]) + z * M[2, 0]) + M[3, 0]
    yv = ((x * M[0, 1] + y * M[1, 1]) + z * M[2, 1]) + M[3, 1]
    t = ((x * M[0, 3] + y * M[1, 3]) + z * M[2, 3]) + M[3, 3]
    zv = ((x * V[0, 2] + y * V[1, 2]) + z * V[2, 2]) + V[3, 2]
    t2 = _eps_denom(t * t)
    td = _eps_denom(t)
    j00 = k(1.0) / td
    j30, j31 = k(-1.0) / t2 * xv, k(-1.0) / t2 * yv
    w0 = [M[r, 0] * j00 + M[r, 3] * j30 for r in range(3)]
    w1 = [M[r, 1] * j00 + M[r, 3] * j31 for r in range(3)]
    if frame is None:
        (ux, uy, uz), (vx, vy, vz) = _frame(n)
    else:
        (ux, uy, uz), (vx, vy, vz) = c(frame[0]).unbind(-1), c(frame[1]).unbind(-1)
    m00 = (ux * w0[0] + uy * w0[1]) + uz * w0[2]
    m01 = (ux * w1[0] + uy * w1[1]) + uz * w1[2]
    m10 = (vx * w0[0] + vy * w0[1]) + vz * w0[2]
    m11 = (vx * w1[0] + vy * w1[1]) + vz * w1[2]
    ps = k(2.0) / k(float(S))
    lp = k(sigma) * (ps * ps)
    g00 = hk * (m00 * m00 + m10 * m10) + lp
    g01 = hk * (m00 * m01 + m10 * m11)
    g11 = hk * (m01 * m01 + m11 * m11) + lp
    detM = m00 * m11 - m01 * m10
    fro = (m00 * m00 + m10 * m10) + (m01 * m01 + m11 * m11)
    # det(h M^T M + lp I) = h^2 det(M)^2 + lp h |M|_F^2 + lp^2: every term non-negative
    detG = (hk * hk) * (detM * detM) + (lp * hk * fro + lp * lp)
    a, cc = g11 / detG, g00 / detG
    b = (-g01 / detG) + (-g01 / detG)
    cut = k(cutoff)
    if radii_form == "den":
        den = _eps_denom(k(4.0) * a * cc - b * b)
        r1 = _sqrt((k(4.0) * a * cut / den).abs().clamp(min=1e-17))
        r0 = _sqrt((k(4.0) * cc * cut / den).abs().clamp(min=1e-17))
    else:
        r0 = _sqrt((g00 * cut).abs().clamp(min=1e-17))
        r1 = _sqrt((g11 * cut).abs().clamp(min=1e-17))
    pi = k(math.pi)
    scaler = detM.abs() / _eps_denom(_sqrt((detG * k(4.0) * pi * pi).abs().clamp(min=1e-17)))
    return {"ndc": torch.stack([xv / t, yv / t, zv], -1), "ellipse_params": torch.stack([a, b, cc], -1),
            "radii": torch.stack([r0, r1], -1), "scaler": scaler,
            "cutoff_threshold": torch.full_like(a, cutoff),
            # (|m00 m11| + |m01 m10|) / sqrt(4 pi^2 det G): the size of the terms det(M) is the difference of
            "scaler_scale": ((m00 * m11).abs() + (m01 * m10).abs()) / _sqrt(detG * k(4.0) * pi * pi)}


RADII_FORM = "g"      # the radii statement splat_setup_point uses (the front end's accuracy table)


def setup32(points, normals, h, V, M, S, sigma=1.0, cutoff=1.0, radii_form=None):
    """The kernel's statements in float32: the yardstick."""
    return _setup_kernel_form(points, normals, h, V, M, S, sigma, cutoff, F32, radii_form or RADII_FORM)


def setup64(points, normals, h, V, M, S, sigma=1.0, cutoff=1.0):
    """The float64 truth for one view: the reference's own statements (oracle.splat_oracle.per_point_info: textbook
    determinant and inverse, harmless in float64) on the float32 inputs, ndc by transform_to_ndc, plus `scaler_scale`
    (what a scaler error is relative to: the scaler itself tends to 0 on grazing rows)."""
    p, n, hk, V, M = (t.to(F64) for t in (points, normals, h, V, M))
    info = SO.per_point_info(p, n, hk, M, S, cutoff=cutoff, sigma=sigma, dtype=F64)
    out = {k: info[k] for k in ("ellipse_params", "radii", "scaler", "cutoff_threshold")}
    out["ndc"] = SO.transform_to_ndc(p, V, M)
    out["scaler_scale"] = _setup_kernel_form(p, n, hk, V, M, S, sigma, cutoff, F64, "g")["scaler_scale"]
    return out


def reference32(points, normals, h, V, M, S, sigma=1.0, cutoff=1.0):
    """The reference's float32 arithmetic (textbook det(G) = g00 g11 - g01^2): printed beside setup32, never a bound."""
    info = SO.per_point_info(points.float(), normals.float(), h.float(), M.float(), S, cutoff=cutoff, sigma=sigma)
    out = {k: info[k] for k in ("ellipse_params", "radii", "scaler")}
    out["ndc"] = SO.transform_to_ndc(points.float(), V.float(), M.float())
    return out


OUTPUTS = ("ndc", "ellipse_params", "radii", "scaler")
QUANTILES = (0.5, 0.9, 0.99, 1.0)


def row_errors(got, truth):
    """{output: (rows,) float64 error}: ndc / ellipse / radii relative to the row's largest |truth|, scaler relative to
    truth["scaler_scale"]."""
    err = {}
    for k in OUTPUTS:
        g = got[k].to(F64).reshape(got[k].shape[0], -1)
        t = truth[k].reshape(g.shape[0], -1)
        scale = truth["scaler_scale"][:, None] if k == "scaler" else t.abs().amax(-1, keepdim=True)
        err[k] = ((g - t).abs() / scale.clamp(min=1e-300)).amax(-1)
    return err


def quantiles(e):
    s = torch.sort(e).values
    n = s.numel()
    return [s[min(n - 1, int(math.ceil(q * n)) - 1)].item() if q < 1.0 else s[-1].item() for q in QUANTILES]


# ---- the case list of the accuracy rule ---------------------------------------------------------------------------
CAMERAS = ("perspective", "orthographic", "off_axis")
NORMALS = ("radial", "grazing", "axis_ties", "short", "long")
SIZES = (1, 64, 1040)
BANDWIDTHS = (0.0, 5e-5, 0.01)
CASE_POINTS = 2000


def camera(kind):
    """(V, M) float32: a look-at view at distance 3 and its full world->NDC matrix.  perspective: 30 degrees;
    orthographic: M[:, 3] = (0, 0, 0, 1); off_axis: the perspective camera with its principal point shifted."""
    V = SO.look_at_view(3.0, 20.0, 35.0)
    Pm = SO.perspective(30.0)
    if kind == "orthographic":
        Pm = torch.zeros(4, 4)
        Pm[0, 0] = Pm[1, 1] = 0.8
        Pm[2, 2] = 1.0 / 99.0
        Pm[3, 2] = -1.0 / 99.0
        Pm[3, 3] = 1.0
    elif kind == "off_axis":
        Pm[2, 0], Pm[2, 1] = 0.3, -0.2
    else:
        assert kind == "perspective"
    return V.contiguous(), (V @ Pm).contiguous()


def case_cloud(normals, V, seed, P=CASE_POINTS):
    """Unit-sphere points and the normals of one class.  grazing: perpendicular to the view ray within 1e-3 .. 1e-6;
    axis_ties: the signed axes, the ties of two or three equal components and (1, 1, 2)-like ties of the two smallest;
    short / long: radial normals of length 0.1 / 10."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=F64), dim=-1)
    if normals in ("radial", "short", "long"):
        nrm = pts * {"radial": 1.0, "short": 0.1, "long": 10.0}[normals]
    elif normals == "grazing":
        C = -(V[3, :3].double() @ V[:3, :3].double().T)                     # the camera centre
        ray = torch.nn.functional.normalize(pts - C, dim=-1)
        side = torch.nn.functional.normalize(torch.cross(ray, torch.randn(P, 3, generator=g, dtype=F64), dim=-1), dim=-1)
        tilt = 10.0 ** (-3.0 - 3.0 * torch.rand(P, 1, generator=g, dtype=F64))
        nrm = torch.nn.functional.normalize(side - tilt * ray, dim=-1)
    else:
        assert normals == "axis_ties"
        base = []
        for a in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 2, 2), (0, 1, 2)):
            for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
                for sx in (1, -1):
                    for sy in (1, -1):
                        for sz in (1, -1):
                            base.append([a[perm[0]] * sx, a[perm[1]] * sy, a[perm[2]] * sz])
        base = torch.unique(torch.tensor(base, dtype=F64), dim=0)
        nrm = base[torch.arange(P) % base.shape[0]]
        nrm = torch.where((torch.arange(P) % 2 == 0)[:, None], nrm, torch.nn.functional.normalize(nrm, dim=-1))
    return pts.float().contiguous(), nrm.float().contiguous()


def setup_cases():
    """[(name, camera, normals, S, h)]: the product the accuracy rule runs over."""
    return [("%s-%s-S%d-h%g" % (c, n, S, h), c, n, S, h) for c in CAMERAS for n in NORMALS for S in SIZES
            for h in BANDWIDTHS]


# ----------------------------------------------------------------------------- gradient to the world points
def _points_backward_terms(points, views, projs, flags, first, src, grad_ndc, dtype):
    """d L / d p = sum over the views a point is rendered in of
         gx (M[j][0] - ndc_x M[j][3]) / t + gy (M[j][1] - ndc_y M[j][3]) / t + gz V[j][2]
    in the kernel's statements (k_splat_points_backward).  -> grad (P,3), sum of |terms| (P,3)."""
    p = points.to(dtype)
    P = p.shape[0]
    grad = torch.zeros(P, 3, dtype=dtype)
    mag = torch.zeros(P, 3, dtype=F64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    one = torch.tensor(1.0, dtype=dtype)
    for v in range(flags.shape[0]):
        sel = flags[v]
        n = int(sel.sum())
        if n == 0:
            continue
        rows = slice(int(first[v]), int(first[v]) + n)
        assert torch.equal(src[rows].long(), torch.nonzero(sel).flatten())
        g = torch.zeros(P, 3, dtype=dtype)
        g[sel] = grad_ndc[rows].to(dtype)
        M, V = projs[v].to(dtype), views[v].to(dtype)
        xv = ((x * M[0, 0] + y * M[1, 0]) + z * M[2, 0]) + M[3, 0]
        yv = ((x * M[0, 1] + y * M[1, 1]) + z * M[2, 1]) + M[3, 1]
        t = ((x * M[0, 3] + y * M[1, 3]) + z * M[2, 3]) + M[3, 3]
        it = one / _eps_denom(t)
        nx, ny = xv * it, yv * it
        g0, g1, g2 = g[:, 0] * it, g[:, 1] * it, g[:, 2]
        for j in range(3):
            t0, t1, t2 = g0 * (M[j, 0] - nx * M[j, 3]), g1 * (M[j, 1] - ny * M[j, 3]), g2 * V[j, 2]
            term = (t0 + t1) + t2
            grad[:, j] = grad[:, j] + torch.where(sel, term, torch.zeros_like(term))
            m = (g0 * M[j, 0]).abs() + (g0 * nx * M[j, 3]).abs() + (g1 * M[j, 1]).abs() + (g1 * ny * M[j, 3]).abs() + t2.abs()
            mag[:, j] += torch.where(sel, m.to(F64), torch.zeros(P, dtype=F64))
    return grad, mag


def points_backward32(points, views, projs, flags, first, src, grad_ndc):
    return _points_backward_terms(points, views, projs, flags, first, src, grad_ndc, F32)[0]


def points_backward64(points, views, projs, flags, first, src, grad_ndc):
    """float64 autograd of [p, 1] M -> (x / w, y / w), z_view = ([p, 1] V)[2], contracted with grad_ndc and summed over
    the views a point is rendered in.  -> grad (P,3) float64, scale (P,) float64 = the point's sum of |terms| (over its
    views and the three components: what a float32 evaluation's error is proportional to)."""
    xd = points.to(F64).clone().requires_grad_(True)
    tot = xd.sum() * 0.0
    for v in range(flags.shape[0]):
        n = int(flags[v].sum())
        rows = slice(int(first[v]), int(first[v]) + n)
        ph = torch.cat([xd[src[rows].long()], torch.ones(n, 1, dtype=F64)], dim=1)
        clip = ph @ projs[v].to(F64)
        zv = (ph @ views[v].to(F64))[:, 2]
        ndc = torch.stack([clip[:, 0] / clip[:, 3], clip[:, 1] / clip[:, 3], zv], dim=1)
        tot = tot + (ndc * grad_ndc[rows].to(F64)).sum()
    tot.backward()
    _, mag = _points_backward_terms(points, views, projs, flags, first, src, grad_ndc, F64)
    return xd.grad, mag.sum(-1)


# ----------------------------------------------------------------------------- isotropic bandwidth
def vrk_h_ref(dists, num, cloud_num=None):
    """h = clamp(0.5 * max of columns 1..6 of the K = 7 squared distances, 5e-5, 0.01) per row (rasterizer.py:375-386),
    every distance replaced by 1e-3 for a cloud of fewer than 7 points.  dists (N, p_stride, 7) float32 as FRNN leaves
    them: a missing neighbour is -1, so a row without any hit gives 0.5 * -1 -> the lower clamp.  -> packed (sum num,)."""
    cloud_num = num if cloud_num is None else cloud_num
    out = []
    for n in range(dists.shape[0]):
        d = dists[n, :int(num[n]), 1:].float().clone()
        if int(cloud_num[n]) < 7:
            d[:] = 1e-3
        m = d.max(dim=-1).values if d.shape[0] else d.new_zeros(0)
        lo, hi = torch.tensor(5e-5, dtype=F32), torch.tensor(0.01, dtype=F32)
        out.append(torch.minimum(torch.maximum(0.5 * m, lo), hi))
    return torch.cat(out) if out else torch.zeros(0)
