"""Compositing (csrc/splat_composite.hip, composite_pixel in csrc/splat_pixel.h) restated in plain float64 numpy:
forward, the explicit backward formulas, the error bounds the GPU tests apply, a float32 restatement in the kernels'
order, and synthetic per-pixel lists.  No autograd: tests/test_composite_cpu.py checks these statements against
oracle/splat_oracle.composite and torch autograd through it.

    w_k = exp(-q_k / 2) s[p_k]   (live slots: p_k >= 0),   A_c = sum_k w_k f_c[p_k],   sw = sum_k w_k
    d = max(sw, eps) (norm_weighted) or 1,   through = norm_weighted and sw > eps
    out_c = A_c / d,   out_C = occupancy
    dL/df_c[p] = sum_{(i,k)->p} g_c w_k / d
    dL/dw_k    = (sum_c g_c f_c[p_k] - [through] sum_c g_c out_c) / d
    dL/dq_k    = -w_k / 2 dL/dw_k,   dL/ds[p] = sum_{(i,k)->p} exp(-q_k / 2) dL/dw_k,   dL/docc = g_C

Everything is vectorised over the pixels with a Python loop over K; arrays are numpy, pixels flattened to (n_pix, ...).
`eps` is the float32 value the kernels receive (EPS below), so both sides clamp at the same number."""
import numpy as np

U = 2.0 ** -24            # float32 unit roundoff
Q_MAX = 9.0               # the generator's largest q
EPS = float(np.float32(1e-4))


def _np(x, dtype=None):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    return x.astype(dtype) if dtype is not None else x


def _lists(idx, q, scaler, feat, dtype):
    idx = _np(idx).astype(np.int64)
    n_pix, K = idx.reshape(-1, idx.shape[-1]).shape
    idx = idx.reshape(n_pix, K)
    live = idx >= 0
    pc = np.where(live, idx, 0)
    q = np.where(live, _np(q, dtype).reshape(n_pix, K), dtype(0))       # dead slots may hold anything, NaN included
    scaler = _np(scaler, dtype).reshape(-1)
    feat = _np(feat, dtype)
    feat = feat.reshape(scaler.shape[0], -1) if feat.size else np.zeros((scaler.shape[0], 0), dtype)
    return idx, live, pc, q, scaler, feat


def forward(idx, q, occ, scaler, feat, norm, eps=EPS):
    """-> dict: image (n_pix, C+1), sw, d, through (n_pix,), S_c (n_pix, C) = sum_k w_k |f_kc| / d, all float64."""
    idx, live, pc, q, scaler, feat = _lists(idx, q, scaler, feat, np.float64)
    n_pix, K = idx.shape
    C = feat.shape[1]
    sw = np.zeros(n_pix)
    A = np.zeros((n_pix, C))
    Sabs = np.zeros((n_pix, C))
    for k in range(K):
        w = np.where(live[:, k], np.exp(-0.5 * q[:, k]) * scaler[pc[:, k]], 0.0)
        f = feat[pc[:, k]]
        A += w[:, None] * f
        Sabs += w[:, None] * np.abs(f)
        sw += w
    if norm:
        d = np.where(sw > eps, sw, eps)
        through = sw > eps
    else:
        d = np.ones(n_pix)
        through = np.zeros(n_pix, bool)
    image = np.concatenate([A / d[:, None], _np(occ, np.float64).reshape(n_pix, 1)], axis=1)
    return {"image": image, "sw": sw, "d": d, "through": through, "S_c": Sabs / d[:, None]}


def _scatter(p, v, P):
    return np.bincount(p, weights=v, minlength=P)


def backward(idx, q, occ, scaler, feat, norm, eps, grad_img):
    """-> dict: grad_features (P,C), grad_q (n_pix,K), grad_scaler (P,), grad_occ (n_pix,) in float64, and the companions
    of the bounds: Gq (n_pix,K) = w_k G_k / 2, Bf (P,C) = sum |g_c| w_k / d, Bs (P,) = sum e_k G_k, with
    G_k = (sum_c |g_c f_kc| + [through] sum_c |g_c| S_c) / d, and n_p (P,) = live fragments that reference point p."""
    fw = forward(idx, q, occ, scaler, feat, norm, eps)
    idx, live, pc, q, scaler, feat = _lists(idx, q, scaler, feat, np.float64)
    n_pix, K = idx.shape
    P, C = feat.shape
    gi = _np(grad_img, np.float64).reshape(n_pix, C + 1)
    g = gi[:, :C]
    d, thr = fw["d"], fw["through"].astype(np.float64)
    go = (g * fw["image"][:, :C]).sum(1)
    go_abs = (np.abs(g) * fw["S_c"]).sum(1)
    out = {"grad_features": np.zeros((P, C)), "grad_q": np.zeros((n_pix, K)), "grad_scaler": np.zeros(P),
           "grad_occ": gi[:, C].copy(), "Gq": np.zeros((n_pix, K)), "Bf": np.zeros((P, C)), "Bs": np.zeros(P),
           "n_p": np.zeros(P, np.int64)}
    for k in range(K):
        m = live[:, k]
        p = pc[m, k]
        e = np.exp(-0.5 * q[m, k])
        w = e * scaler[p]
        f = feat[p]
        gw = ((g[m] * f).sum(1) - thr[m] * go[m]) / d[m]
        G = (np.abs(g[m] * f).sum(1) + thr[m] * go_abs[m]) / d[m]
        out["grad_q"][m, k] = -0.5 * w * gw
        out["Gq"][m, k] = 0.5 * w * G
        out["grad_scaler"] += _scatter(p, e * gw, P)
        out["Bs"] += _scatter(p, e * G, P)
        out["n_p"] += np.bincount(p, minlength=P)
        for c in range(C):
            out["grad_features"][:, c] += _scatter(p, g[m, c] * w / d[m], P)
            out["Bf"][:, c] += _scatter(p, np.abs(g[m, c]) * w / d[m], P)
    out["forward"] = fw
    return out


def bounds(bw, K, C, chunks=1):
    """The derived bounds (u = 2^-24; expf within 1 ulp, the product -q/2, K-term sums in any fixed order, n_p-term sums
    in any order for the float atomics).  `chunks`: composite() above 8 channels adds the chunks' grad_q, one more
    rounding of the companion per boundary."""
    fw = bw["forward"]
    n_p = bw["n_p"].astype(np.float64)
    return {"image": image_bound(fw, K),
            "grad_q": (2 * K + C + 16 + (chunks - 1)) * U * bw["Gq"],
            "grad_features": (n_p + 2 * K + 16)[:, None] * U * bw["Bf"],
            "grad_scaler": (n_p + 2 * K + C + 16) * U * bw["Bs"]}


def image_bound(fw, K):
    return (K + 8 + Q_MAX / 2) * U * fw["S_c"]


def ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound; where the bound is 0 the values must be equal (else inf).  A
    non-finite `got` gives inf."""
    got = _np(got, np.float64).reshape(ref.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


def restate_f32(idx, q, occ, scaler, feat, norm, eps, grad_img, seed=0):
    """The kernels' statements in float32 and in their order (k ascending, sums ((.)+.)+., every product and sum
    rounded on its own), the per-point scatter accumulated one term at a time in a shuffled order, as atomics arrive.
    -> dict image, grad_features, grad_q, grad_scaler, grad_occ (float32)."""
    f32 = np.float32
    idx, live, pc, q, scaler, feat = _lists(idx, q, scaler, feat, f32)
    n_pix, K = idx.shape
    P, C = feat.shape
    gi = _np(grad_img, f32).reshape(n_pix, C + 1)
    g = gi[:, :C]
    eps = f32(eps)
    sw = np.zeros(n_pix, f32)
    acc = np.zeros((n_pix, C), f32)
    for k in range(K):
        m = live[:, k]
        w = np.exp(f32(-0.5) * q[:, k]) * scaler[pc[:, k]]
        acc = np.where(m[:, None], acc + w[:, None] * feat[pc[:, k]], acc)
        sw = np.where(m, sw + w, sw)
    if norm:
        d = np.where(sw > eps, sw, eps).astype(f32)
        through = sw > eps
    else:
        d = np.ones(n_pix, f32)
        through = np.zeros(n_pix, bool)
    out = acc / d[:, None]
    image = np.concatenate([out, _np(occ, f32).reshape(n_pix, 1)], axis=1)
    go = np.zeros(n_pix, f32)
    for c in range(C):
        go = go + g[:, c] * out[:, c]
    go = np.where(through, go, f32(0))
    gq = np.zeros((n_pix, K), f32)
    sp, sv, fp, fv = [], [], [], []
    for k in range(K):
        m = live[:, k]
        p = pc[m, k]
        e = np.exp(f32(-0.5) * q[m, k])
        w = e * scaler[p]
        f = feat[p]
        gw = np.zeros(p.shape[0], f32)
        for c in range(C):
            gw = gw + g[m, c] * f[:, c]
        gw = (gw - go[m]) / d[m]
        gq[m, k] = f32(-0.5) * w * gw
        sp.append(p)
        sv.append(e * gw)
        fp.append(p)
        fv.append(g[m] * w[:, None] / d[m][:, None])
    rng = np.random.default_rng(seed)
    sp, sv, fp, fv = np.concatenate(sp), np.concatenate(sv), np.concatenate(fp), np.concatenate(fv)
    order = rng.permutation(sp.shape[0])
    gs = np.zeros(P, f32)
    np.add.at(gs, sp[order], sv[order].astype(f32))
    gf = np.zeros((P, C), f32)
    for c in range(C):
        order = rng.permutation(fp.shape[0])
        np.add.at(gf[:, c], fp[order], fv[order, c].astype(f32))
    return {"image": image, "grad_features": gf, "grad_q": gq, "grad_scaler": gs, "grad_occ": gi[:, C].copy()}


def fragments(n_pix, K, C, P, seed, live=0.7, scaler_hi=1.0, empty=0.0, dead_q=float("nan"), hot_point=None):
    """Synthetic per-pixel lists, no rasteriser involved -> dict of numpy arrays:
    idx (n_pix,K) int32 uniform in [0,P) on a `live` share of the slots, -1 elsewhere and NOT front-packed (an `empty`
    share of the pixels has no live slot at all); every point is referenced at least once; hot_point: slot 0 of every
    pixel lists that point.  q (n_pix,K) float32 uniform in [0, Q_MAX], `dead_q` (NaN) in the dead slots.
    occ (n_pix,) float32 uniform.  scaler (P,) uniform in (0, scaler_hi].  feat (P,C), grad_img (n_pix,C+1) normal."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, P, size=(n_pix, K)).astype(np.int32)
    alive = rng.random((n_pix, K)) < live
    if empty > 0:
        alive &= (rng.random(n_pix) >= empty)[:, None]
    if hot_point is not None:
        alive[:, 0] = True
        idx[:, 0] = hot_point
    else:
        slots = np.flatnonzero(alive.reshape(-1))
        assert slots.shape[0] >= P, "fewer live slots than points"
        idx.reshape(-1)[rng.choice(slots, size=P, replace=False)] = np.arange(P, dtype=np.int32)
    idx[~alive] = -1
    q = (rng.random((n_pix, K)) * Q_MAX).astype(np.float32)
    q[~alive] = dead_q
    scaler = ((1.0 - rng.random(P)) * scaler_hi).astype(np.float32)
    scaler = np.maximum(scaler, np.float32(scaler_hi) * np.float32(2.0 ** -24))
    return {"idx": idx, "q": q, "occ": rng.random(n_pix).astype(np.float32), "scaler": scaler,
            "feat": rng.standard_normal((P, C)).astype(np.float32),
            "grad_img": rng.standard_normal((n_pix, C + 1)).astype(np.float32)}


# ------------------------------------------------------------------------------------------------ the GPU file's sets
# name -> (fragments() arguments, the norm_weighted values run on it).  tests/test_composite_gpu.py draws every list it
# composites from here and tests/test_composite_cpu.py asserts the input conditions on each (clamp decision not within
# 1e-3 of eps, live share in [0.5, 0.9], every point referenced) and the float32 restatement's ratios.
FORM_K = (1, 3, 4, 6, 8, 9, 33, 150)
FORM_C = (0, 1, 3, 4, 8)
N_FORM = 1 * 37 * 29
N_STRIDE = 1048576 + 300
CLAMP_HI = {1: 2.0e-3, 8: 2.0e-4}       # scaler_hi that puts 30 % .. 70 % of the non-empty pixels at sw <= eps


def form_set(K, C):
    return fragments(N_FORM, K, C, 64, seed=1000 * K + C)


def clamp_set(K):
    return fragments(N_FORM, K, 3, 64, seed=7 + K, scaler_hi=CLAMP_HI[K], empty=0.15)


def garbage_set(K, dead_q=float("nan")):
    return fragments(N_FORM, K, 3, 64, seed=40 + K, dead_q=dead_q)


def contention_set():
    return fragments(20000, 8, 3, 500, seed=5, hot_point=0)


def stride_set():
    return fragments(N_STRIDE, 1, 1, 16, seed=6)


def subset_set():
    return fragments(N_FORM, 6, 3, 64, seed=8)


def wide_set(K):
    return fragments(N_FORM, K, 16, 64, seed=16 + K)


def all_sets():
    """(name, K, C, set, norms, contention) for every synthetic set the GPU file composites."""
    out = []
    for K in FORM_K:
        for C in FORM_C:
            out.append(("form K=%d C=%d" % (K, C), K, C, form_set(K, C), (True, False), False))
    for K in (1, 8):
        out.append(("clamp K=%d" % K, K, 3, clamp_set(K), (True,), False))
    for K in (4, 6, 8):
        out.append(("garbage K=%d" % K, K, 3, garbage_set(K), (True, False), False))
    out.append(("contention", 8, 3, contention_set(), (True,), True))
    out.append(("stride", 1, 1, stride_set(), (True, False), False))
    out.append(("subsets", 6, 3, subset_set(), (True,), False))
    for K in (6, 8):
        out.append(("wide K=%d" % K, K, 16, wide_set(K), (True, False), False))
    return out
