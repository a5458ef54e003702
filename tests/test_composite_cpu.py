"""tests/composite_oracle.py checked on the CPU: its float64 forward against oracle/splat_oracle.composite, its explicit
backward against torch autograd through that, the input conditions of every set tests/test_composite_gpu.py composites,
and the float32 restatement (kernel order, shuffled scatter) against the derived bounds with a factor 2 to spare."""
import numpy as np
import pytest
import torch

import composite_oracle as CO
from oracle import splat_oracle as SO


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 0.0 if a.size == 0 else float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _so_composite(s, norm, eps, grad=False):
    """oracle/splat_oracle.composite on a synthetic set in float64 (dead slots' q zeroed: the gradient of a masked NaN
    is NaN in autograd, and the kernels never read those slots)."""
    n_pix, K = s["idx"].shape
    idx = torch.from_numpy(s["idx"]).view(1, n_pix, 1, K)
    q = torch.from_numpy(np.where(s["idx"] >= 0, s["q"], 0).astype(np.float64)).view(1, n_pix, 1, K).requires_grad_(grad)
    occ = torch.from_numpy(s["occ"].astype(np.float64)).view(1, n_pix, 1).requires_grad_(grad)
    scal = torch.from_numpy(s["scaler"].astype(np.float64)).requires_grad_(grad)
    feat = torch.from_numpy(s["feat"].astype(np.float64)).requires_grad_(grad)
    fr = SO.PointFragments(idx, None, q, SO.gather_scaler(scal, idx), occ)
    img = SO.composite(fr, feat, norm_weighted=norm, eps=eps)
    return img, (q, occ, scal, feat)


CROSS = [("form", 1, 3), ("form", 4, 0), ("form", 6, 4), ("form", 8, 8), ("form", 33, 1), ("clamp", 1, 3), ("clamp", 8, 3),
         ("wide", 6, 16)]


def _cross_set(kind, K, C):
    return {"form": lambda: CO.form_set(K, C), "clamp": lambda: CO.clamp_set(K), "wide": lambda: CO.wide_set(K)}[kind]()


@pytest.mark.parametrize("kind,K,C", CROSS)
@pytest.mark.parametrize("norm", [True, False])
def test_forward_is_the_splat_oracles_composite(kind, K, C, norm):
    s = _cross_set(kind, K, C)
    fw = CO.forward(s["idx"], s["q"], s["occ"], s["scaler"], s["feat"], norm, CO.EPS)
    ref, _ = _so_composite(s, norm, CO.EPS)
    ref = ref.reshape(-1, C + 1).numpy()
    assert fw["image"].shape == ref.shape and np.isfinite(fw["image"]).all()
    assert _rel(fw["image"], ref) <= 1e-14
    assert np.array_equal(fw["image"][:, C], s["occ"].astype(np.float64))


@pytest.mark.parametrize("kind,K,C", CROSS)
@pytest.mark.parametrize("norm", [True, False])
def test_backward_is_autograd_of_the_splat_oracles_composite(kind, K, C, norm):
    """clamp K=1 / K=8: pixels with sw <= eps (no second term) and empty pixels; K=1: the exact cancellation."""
    s = _cross_set(kind, K, C)
    bw = CO.backward(s["idx"], s["q"], s["occ"], s["scaler"], s["feat"], norm, CO.EPS, s["grad_img"])
    img, (q, occ, scal, feat) = _so_composite(s, norm, CO.EPS, grad=True)
    img.backward(torch.from_numpy(s["grad_img"].astype(np.float64)).view(img.shape))
    if kind == "clamp" and norm:
        fw = bw["forward"]
        assert (fw["sw"] == 0).any() and ((fw["sw"] > 0) & ~fw["through"]).any() and fw["through"].any()
    # relative to the largest companion (the sum of the terms' magnitudes): at K = 1 the true gradient is a rounding
    # residue of either side, and "relative to itself" would compare two of those
    for got, ref, comp in ((bw["grad_q"], q.grad.reshape(-1, K), bw["Gq"]), (bw["grad_scaler"], scal.grad, bw["Bs"]),
                           (bw["grad_features"], feat.grad, bw["Bf"])):
        assert got.size == 0 or np.abs(got - ref.numpy()).max() <= 1e-12 * comp.max()
    assert np.array_equal(bw["grad_occ"], occ.grad.reshape(-1).numpy())
    if K == 1 and norm:                      # out = f on a `through` pixel: dL/dw vanishes identically
        thr = bw["forward"]["through"]
        assert thr.any() and np.abs(bw["grad_q"][thr]).max() <= 1e-12 * np.abs(bw["Gq"][thr]).max()


def test_clamp_sets_share_and_contention_count():
    for K in (1, 8):
        s = CO.clamp_set(K)
        fw = CO.forward(s["idx"], s["q"], s["occ"], s["scaler"], s["feat"], True, CO.EPS)
        nonempty = (s["idx"] >= 0).any(1)
        share = float((~fw["through"])[nonempty].mean())
        print("clamp K=%d: %.3f of the non-empty pixels at sw <= eps, %.3f of the pixels empty" % (K, share, 1 - nonempty.mean()))
        assert 0.3 <= share <= 0.7
        assert (~nonempty).mean() >= 0.10
    s = CO.contention_set()
    assert np.bincount(s["idx"][s["idx"] >= 0], minlength=500)[0] >= 20000
    for K in (4, 6, 8):                      # the two dead-slot conventions differ in the dead slots of q and nowhere else
        a, b = CO.garbage_set(K), CO.garbage_set(K, dead_q=-1.0)
        dead = a["idx"] < 0
        assert np.isnan(a["q"][dead]).all() and (b["q"][dead] == -1).all() and np.array_equal(a["q"][~dead], b["q"][~dead])
        assert all(np.array_equal(a[k], b[k]) for k in a if k != "q")


def test_input_conditions_and_f32_restatement_within_half_the_bounds():
    """Every synthetic set of the GPU file: the clamp decision is not within 1e-3 of eps on any pixel, the live share is
    in [0.5, 0.9], every point is referenced (the contention set aside), dead slots are not front-packed and hold NaN;
    and the float32 restatement sits within half of each bound, element by element."""
    worst = {"image": 0.0, "grad_q": 0.0, "grad_features": 0.0, "grad_scaler": 0.0}
    for name, K, C, s, norms, contention in CO.all_sets():
        idx = s["idx"]
        live = idx >= 0
        assert idx.dtype == np.int32 and idx.shape[1] == K and s["feat"].shape[1] == C
        assert 0.5 <= live.mean() <= 0.9, name
        assert idx.max() < s["scaler"].shape[0] and idx.min() == -1
        assert np.isnan(s["q"][~live]).all() and (s["q"][live] >= 0).all() and (s["q"][live] <= CO.Q_MAX).all()
        assert (s["scaler"] > 0).all() and np.isfinite(s["scaler"]).all()
        if K > 1:                            # a live slot behind a dead one somewhere: the lists are not front-packed
            assert (live[:, 1:] & ~live[:, :-1]).any(), name
        n_p = np.bincount(idx[live], minlength=s["scaler"].shape[0])
        if not contention:
            assert n_p.min() >= 1, name
        for norm in norms:
            bw = CO.backward(idx, s["q"], s["occ"], s["scaler"], s["feat"], norm, CO.EPS, s["grad_img"])
            fw = bw["forward"]
            assert np.array_equal(bw["n_p"], n_p)
            if norm:
                assert np.abs(fw["sw"] / CO.EPS - 1).min() >= 1e-3, name
            b = CO.bounds(bw, K, C)
            r32 = CO.restate_f32(idx, s["q"], s["occ"], s["scaler"], s["feat"], norm, CO.EPS, s["grad_img"], seed=K + C)
            assert np.array_equal(r32["grad_occ"], s["grad_img"][:, C])
            for k, ref in (("image", fw["image"][:, :C]), ("grad_q", bw["grad_q"]), ("grad_features", bw["grad_features"]),
                           ("grad_scaler", bw["grad_scaler"])):
                got = r32[k][:, :C] if k == "image" else r32[k]
                r = CO.ratio(got, ref, b[k])
                assert r <= 0.5, (name, norm, k, r)
                worst[k] = max(worst[k], r)
    print("float32 restatement, largest error / bound: " + ", ".join("%s %.3f" % kv for kv in worst.items()))
