"""One auto-decoder training step's forward + backward of a latent-conditioned SIREN with ONE CODE PER CLOUD, on the package's
kernels (siren_forward(lengths=) under grad: iso_siren_sdf_grad_coded, then iso_sirencode_backward -- the sweeps with the
table row of every point, the per-code sums of zbar_0) against the torch route the same clouds take without the keyword
(padded (U, P, 3) points with c (U, C): model.forward on [c, x] and autograd.grad(create_graph=True), the second backward
through it), and beside the fused route with one code for all points (iso_sirengrad_backward_b0), the path that existed.
The loss is mean(f^2) + 0.01 mean((|g| - 1)^2); gradients go to every parameter and every code.
Network: SIREN 4 x 256 (three hidden layers), C = 256; sizes: 24 000 points and 262 144; U in {2, 8, 64}, equal rows.
Protocol of tools/siren_backward_timing.py: every timing is the median of 10 device-event timed calls after 2 warm-up calls;
the figure reported is the median over `--rounds` alternating rounds, with the spread.
Writes one JSON document (times in ms) to --out and prints it.
usage: python tools/siren_rowcodes_timing.py [--rounds 3] [--sizes 24000,262144] [--codes 2,8,64]
                                             [--out profiles/siren_rowcodes_timing.json]"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tools_common import timeit  # noqa: E402
from iso_points_amd.sdf_models import Siren, _torch_forward, siren_forward  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="24000,262144")
    ap.add_argument("--codes", default="2,8,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siren_rowcodes_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/siren_rowcodes_timing.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    H, L, C = 256, 3, 256
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "hidden": H, "n_hidden": L, "c_dim": C, "cases": []}
    torch.manual_seed(0)
    net = Siren(hidden_size=H, n_layers=L, c_dim=C).to(dev)
    params = list(net.parameters())
    for n in (int(s) for s in a.sizes.split(",")):
        for U in (int(s) for s in a.codes.split(",")):
            assert n % U == 0, "equal rows"
            pts = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(n), device=dev) * 2 - 1
            codes = (torch.randn(U, C, generator=torch.Generator(device=dev).manual_seed(U), device=dev) * 0.01).requires_grad_(True)
            lengths = [n // U] * U

            def fused_fwd():
                return siren_forward(net, pts, c=codes, lengths=lengths)

            def torch_fwd():
                f, g = _torch_forward(net, pts.view(U, n // U, 3), codes, True, True)
                return f.reshape(-1), g.reshape(-1, 3)

            def one_code_fwd():
                return siren_forward(net, pts, c=codes[:1])

            def step(forward):
                for t in params + [codes]:
                    t.grad = None
                f, g = forward()
                ((f ** 2).mean() + 0.01 * ((g.norm(dim=-1) - 1) ** 2).mean()).backward()
            # faster and different is not faster: every gradient against torch's, relative to its largest entry
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)        # the fused routes do not warn of a torch route
                step(torch_fwd)
                want = [t.grad.clone() for t in params + [codes]]
                step(fused_fwd)
                err = max(((t.grad - w).abs().max() / w.abs().max().clamp_min(1e-30)).item()
                          for t, w in zip(params + [codes], want))
                step(one_code_fwd)
            assert err < 1e-3, err
            t = {"torch": [], "fused": [], "fused_one_code": [], "fused_forward": []}
            for _ in range(a.rounds):
                t["torch"].append(timeit(lambda: step(torch_fwd)))
                t["fused"].append(timeit(lambda: step(fused_fwd)))
                t["fused_one_code"].append(timeit(lambda: step(one_code_fwd)))
                t["fused_forward"].append(timeit(fused_fwd))
            c = {"points": n, "codes": U, "max_rel_grad_diff": err}
            for k, v in t.items():
                v = sorted(v)
                c[k + "_ms"] = round(v[len(v) // 2], 4)
                c[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
            c["fused_backward_ms"] = round(c["fused_ms"] - c["fused_forward_ms"], 4)
            c["speedup"] = round(c["torch_ms"] / c["fused_ms"], 2)
            c["over_one_code"] = round(c["fused_ms"] / c["fused_one_code_ms"], 3)
            res["cases"].append(c)
            print(c, file=sys.stderr, flush=True)
    text = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
