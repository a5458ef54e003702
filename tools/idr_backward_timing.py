"""One training step's forward + backward of the IDR SDF on the package's kernels (idr_forward under grad: the fused
evaluation, then iso_idrgrad_backward: both sweeps with one tangent column per point on the staged f32 tile GEMM, dW on the
f32 matrix instruction) against eager float32 torch autograd of the same module on the same GPU (autograd.grad with
create_graph=True for the normals, then the second backward through it).
The loss is mean(f^2) + 0.01 mean((|g| - 1)^2); gradients go to every parameter (weight norm's g and v, the biases).
Shape: the reference's default, 8 x 512 softplus layers, skip 4, 6 frequencies; sizes: 24 000 points and 262 144.
Protocol of tools/siren_backward_timing.py: every timing is the median of 10 device-event timed calls after 2 warm-up
calls; the figure reported is the median over `--rounds` alternating rounds, with the spread.  "fused_forward_ms" is the
forward alone under grad (the autograd function's forward), so backward = fused - fused_forward.
Writes one JSON document (times in ms) to --out and prints it.
usage: python tools/idr_backward_timing.py [--rounds 3] [--sizes 24000,262144] [--out profiles/idr_backward_timing.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.sdf_models import idr_forward  # noqa: E402
from oracle.iso_oracle import IdrSDF  # noqa: E402

# 6 products of the weights per point and column pair = 5.8 TFLOP at 262 144 points: four in the sweep at the ~60 TFLOP/s the
# staged f32 step kernel reaches with one workgroup per CU (65 ms), two in dW at k_texgrad_tn's 56 TFLOP/s (35 ms), and the
# fused forward (10 ms).  Nobody had measured this when the figure was written down.
PREDICTED_MS_AT_262144 = 110.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="24000,262144")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idr_backward_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/idr_backward_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    H, NL, SKIP, NF = 512, 8, 4, 6
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "hidden": H, "n_layers": NL, "skip": SKIP, "n_freq": NF,
           "predicted_fused_ms_at_262144": PREDICTED_MS_AT_262144, "cases": []}
    torch.manual_seed(0)
    net = IdrSDF(hidden_size=H, n_layers=NL, skip_in=(SKIP,), num_frequencies=NF)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.01 * torch.randn_like(p))
    net = net.to(dev)
    params = list(net.parameters())
    D0 = 3 + 6 * NF
    macs = D0 * H + (NL - 2) * H * H + (H - D0) * H + H
    for n in (int(s) for s in a.sizes.split(",")):
        pts = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(n), device=dev) * 2 - 1

        def eager_fwd():
            x = pts.detach().requires_grad_(True)
            f = net(x).sdf.squeeze(-1)
            g = torch.autograd.grad(f, x, torch.ones_like(f), create_graph=True)[0]
            return f, g

        def fused_fwd():
            return idr_forward(net, pts)

        def step(forward):
            for t in params:
                t.grad = None
            f, g = forward()
            ((f ** 2).mean() + 0.01 * ((g.norm(dim=-1) - 1) ** 2).mean()).backward()
        # faster and different is not faster: every gradient against eager's, relative to its largest entry
        step(eager_fwd)
        want = [t.grad.clone() for t in params]
        step(fused_fwd)
        err = max(((t.grad - w).abs().max() / w.abs().max().clamp_min(1e-30)).item() for t, w in zip(params, want))
        assert err < 1e-3, err
        t = {"eager": [], "fused": [], "eager_forward": [], "fused_forward": []}
        for _ in range(a.rounds):
            t["eager"].append(timeit(lambda: step(eager_fwd)))
            t["fused"].append(timeit(lambda: step(fused_fwd)))
            t["eager_forward"].append(timeit(eager_fwd))
            t["fused_forward"].append(timeit(fused_fwd))
        c = {"points": n, "max_rel_weight_grad_diff": err}
        for k, v in t.items():
            v = sorted(v)
            c[k + "_ms"] = round(v[len(v) // 2], 4)
            c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        c["fused_backward_ms"] = round(c["fused_ms"] - c["fused_forward_ms"], 4)
        c["eager_backward_ms"] = round(c["eager_ms"] - c["eager_forward_ms"], 4)
        # the backward: two columns forward, two reverse, and dW over 2 n rows = 6 products of the weights per point
        c["fused_backward_tflops"] = round(6 * 2.0 * macs * n / (c["fused_backward_ms"] * 1e-3) / 1e12, 1)
        c["speedup"] = round(c["eager_ms"] / c["fused_ms"], 2)
        res["cases"].append(c)
        print(c, file=sys.stderr, flush=True)
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
