"""The fused texture network (iso_points_amd.texture.texture_rgb: weight packing + one forward kernel per call) against
the eager float32 torch forward of the same module on the same GPU, input assembly included (texture_rows + decoder.forward:
the only way to shade without the kernel).
Sizes: 24 000 points (the reference's working set of iso-points) and 262 144 (one 512^2 view, every ray a hit).
Shapes: the reference's default 4 x 512 with c_dim 256 and 4 frequencies, and the same without a code.
Every timing is the median of 10 device-event timed calls after 2 warm-up calls; the figure reported is the median over
`--rounds` alternating rounds, with the spread.  "fused_kernel_ms" re-uses one packed image (the kernel alone), "fused_ms" packs
on every call as texture_rgb does by default.  TFLOP/s are f32-equivalent (2 flop per weight and point) for the fused call
with packing, `frac` against the 839 TFLOP/s ceiling of DESIGN.md 3.1 (fp16 dense / 3).
Prints one JSON line (times in ms).
usage: python tools/texture_timing.py [--rounds 3] [--sizes 24000,262144]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.texture import PackedTexture, RenderingNetwork, texture_rgb, texture_rows  # noqa: E402

CEILING_TFLOPS = 839.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="24000,262144")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/texture_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    for c_dim in (256, 0):
        torch.manual_seed(c_dim)
        net = RenderingNetwork(dim=9, c_dim=c_dim, hidden_size=512, n_layers=4, weight_norm=True, num_frequencies=4).to(dev)
        macs = net.dim * 512 + 3 * 512 * 512 + 512 * 3
        for n in (int(s) for s in a.sizes.split(",")):
            g = torch.Generator(device=dev).manual_seed(n)
            pts = torch.rand(n, 3, generator=g, device=dev) * 2 - 1
            nrm = torch.randn(n, 3, generator=g, device=dev)
            codes = torch.randn(n, c_dim, generator=g, device=dev) if c_dim else None
            cam = torch.tensor([[0.0, 0.5, -3.0]], device=dev)

            def eager():
                with torch.no_grad():
                    return net(texture_rows(net, pts, nrm, cam), c=codes).rgb
            held = PackedTexture(net, dev)
            # faster and different is not faster
            err = (texture_rgb(net, pts, nrm, codes, cam) - eager()).abs().max().item()
            assert err < 1e-5, err
            t = {"eager": [], "fused": [], "fused_kernel": []}
            for _ in range(a.rounds):
                t["eager"].append(timeit(eager))
                t["fused"].append(timeit(lambda: texture_rgb(net, pts, nrm, codes, cam)))
                t["fused_kernel"].append(timeit(lambda: texture_rgb(net, pts, nrm, codes, cam, packed=held)))
            c = {"c_dim": c_dim, "points": n, "max_abs_diff": err}
            for k, v in t.items():
                v = sorted(v)
                c[k + "_ms"] = round(v[len(v) // 2], 4)
                c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
            for k in ("eager", "fused", "fused_kernel"):
                c[k + "_evals_per_s"] = round(n / (c[k + "_ms"] * 1e-3))
                c[k + "_tflops"] = round(2.0 * macs * n / (c[k + "_ms"] * 1e-3) / 1e12, 1)
            c["fused_frac_of_ceiling"] = round(c["fused_tflops"] / CEILING_TFLOPS, 3)
            c["speedup"] = round(c["eager_ms"] / c["fused_ms"], 2)
            res["cases"].append(c)
            print(c, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
