"""Forward + backward of the texture network on the package's kernels (texture_rgb under grad: the fused forward kernel,
then iso_texgrad_backward: recompute and reverse sweep as split-fp16 tile kernels, dx_0 and dW on the f32 matrix
instruction) against eager float32 torch autograd of the same module on
the same GPU, input assembly included.  The loss is sum(rgb * G); gradients go to every parameter, the codes, the normals
and the points.
Sizes: 24 000 points and 262 144; shapes: the reference's default 4 x 512 with 4 frequencies, c_dim 256 and 0.
Protocol of tools/texture_timing.py: every timing is the median of 10 device-event timed calls after 2 warm-up calls; the
figure reported is the median over `--rounds` alternating rounds, with the spread.  "fused_forward_ms" is the forward alone
under grad (the autograd function's forward), so backward = fused - fused_forward.
Writes one JSON document (times in ms) to --out and prints it.
usage: python tools/texture_backward_timing.py [--rounds 3] [--sizes 24000,262144] [--out profiles/texture_backward_timing.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.texture import RenderingNetwork, texture_rgb, texture_rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="24000,262144")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_backward_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/texture_backward_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    for c_dim in (256, 0):
        torch.manual_seed(c_dim)
        net = RenderingNetwork(dim=9, c_dim=c_dim, hidden_size=512, n_layers=4, weight_norm=True, num_frequencies=4).to(dev)
        macs = net.dim * 512 + 3 * 512 * 512 + 512 * 3
        for n in (int(s) for s in a.sizes.split(",")):
            g = torch.Generator(device=dev).manual_seed(n)
            pts = (torch.rand(n, 3, generator=g, device=dev) * 2 - 1).requires_grad_(True)
            nrm = torch.randn(n, 3, generator=g, device=dev).requires_grad_(True)
            codes = torch.randn(n, c_dim, generator=g, device=dev).requires_grad_(True) if c_dim else None
            cam = torch.tensor([[0.0, 0.5, -3.0]], device=dev)
            G = torch.randn(n, 3, generator=g, device=dev)
            leaves = [t for t in (pts, nrm, codes) if t is not None] + list(net.parameters())

            def step(forward):
                for t in leaves:
                    t.grad = None
                (forward() * G).sum().backward()

            def eager_fwd():
                return net(texture_rows(net, pts, nrm, cam), c=codes).rgb

            def fused_fwd():
                return texture_rgb(net, pts, nrm, codes, cam)
            # A ReLU within rounding of 0 flips between two float32 paths, and one flipped point moves a weight gradient (a
            # sum of terms of both signs) by 1 / sqrt(n) of its largest entry: the points with a pre-activation on the fence
            # get no loss weight.  The tests' oracle (tests/texture_backward_oracle.py) filters at 1e-6 of max|z| on float64
            # pre-activations; here they are eager's float32 ones on the GPU, themselves off by ~1e-6, so the fence is 1e-5
            # wide.  That takes the loss weight of 8-9 % of the rows; the kernels' work does not depend on G, so the
            # timing is not affected.
            with torch.no_grad():
                x = texture_rows(net, pts, nrm, cam)
                x = x if codes is None else torch.cat([codes, x], dim=-1)
                keep = torch.ones(n, dtype=torch.bool, device=dev)
                for l in range(net.num_layers - 2):
                    z = getattr(net, "lin%d" % l)(x)
                    keep &= (z.abs() >= 1e-5 * z.abs().max()).all(dim=1)
                    x = torch.relu(z)
                G = G * keep[:, None]
            # faster and different is not faster: every gradient against eager's, relative to its largest entry
            step(eager_fwd)
            want = [t.grad.clone() for t in leaves]
            step(fused_fwd)
            err = max(((t.grad - w).abs().max() / w.abs().max().clamp_min(1e-30)).item() for t, w in zip(leaves, want))
            off = 1.0 - keep.float().mean().item()
            assert err < 1e-4 and off < 0.2, (err, off)
            t = {"eager": [], "fused": [], "eager_forward": [], "fused_forward": []}
            for _ in range(a.rounds):
                t["eager"].append(timeit(lambda: step(eager_fwd)))
                t["fused"].append(timeit(lambda: step(fused_fwd)))
                t["eager_forward"].append(timeit(eager_fwd))
                t["fused_forward"].append(timeit(fused_fwd))
            c = {"c_dim": c_dim, "points": n, "max_rel_weight_grad_diff": err, "fraction_of_rows_without_loss_weight": off}
            for k, v in t.items():
                v = sorted(v)
                c[k + "_ms"] = round(v[len(v) // 2], 4)
                c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
            c["fused_backward_ms"] = round(c["fused_ms"] - c["fused_forward_ms"], 4)
            c["eager_backward_ms"] = round(c["eager_ms"] - c["eager_forward_ms"], 4)
            # forward + recompute + reverse + dW: 2 flop per weight and point, four times
            c["fused_tflops"] = round(4 * 2.0 * macs * n / (c["fused_ms"] * 1e-3) / 1e12, 1)
            c["speedup"] = round(c["eager_ms"] / c["fused_ms"], 2)
            res["cases"].append(c)
            print(c, file=sys.stderr, flush=True)
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
