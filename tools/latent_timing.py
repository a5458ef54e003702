"""Cost of the latent-conditioned SIREN route: ms per UniformProjection._project_points call (SIREN 3 -> 256 x 3 -> 1,
T = 10, default stopping tolerance) on 1 M points around the unit sphere for
  uncoded        the FOLDED network of one code: Siren(c_dim = 0) with the coded model's xyz columns and b0 := that
                 code's table row -- the same bits and the same survivors per iteration as one_code, so the two times
                 differ by the cost of the coded kernels and the fold alone          iso_project_siren
  one_code       Siren(c_dim = 32), c of shape (C,)                 iso_siren_fold_codes + iso_project_siren_coded
  four_clouds    Siren(c_dim = 32), 4 clouds of 250 k, c (4, C)     the same with code_of (other codes: other survivors)
  generic_100k   Siren(c_dim = 32), per-point codes (P, C): the generic torch route, at 100 k points (for contrast; with
                 a stopping tolerance no point meets, so that the loop never compacts the points away from their codes)
Median of 7 timed calls (HIP events) after 2 warm-up calls.  Prints one JSON line.
usage: python tools/latent_timing.py"""
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iso_points_amd.levelset_sampling import UniformProjection  # noqa: E402
from iso_points_amd.sdf_models import PackedSiren, Siren  # noqa: E402


def ms_per_call(fn, warm=2, rep=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def sphere(P, B, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.nn.functional.normalize(torch.randn(B, P // B, 3, generator=g), dim=-1)
    return (p + 0.05 * (torch.rand(B, P // B, 3, generator=g) - 0.5)).to(dev)


def main():
    dev = torch.device("cuda:0")
    C, P = 32, 1_000_000
    torch.manual_seed(0)
    coded = Siren(hidden_size=256, n_layers=3, c_dim=C).to(dev)
    codes = 0.1 * torch.randn(4, C, device=dev)
    plain = Siren(hidden_size=256, n_layers=3).to(dev)
    with torch.no_grad():
        plain.load_state_dict({k: v for k, v in coded.state_dict().items() if not k.startswith("net.0.")}, strict=False)
        plain.net[0].linear.weight.copy_(coded.net[0].linear.weight[:, C:])
        plain.net[0].linear.bias.copy_(PackedSiren(coded, dev).fold(codes[:1])[0])
    up = UniformProjection()
    one = sphere(P, 1, dev)
    four = sphere(P, 4, dev)
    n1 = torch.tensor([P], device=dev)
    n4 = torch.tensor([P // 4] * 4, device=dev)
    out = {"points": P, "hidden": 256, "n_hidden": 3, "c_dim": C, "T": 10}
    out["uncoded_ms"] = ms_per_call(lambda: up._project_points(plain, one, n1, proj_max_iters=10))
    out["one_code_ms"] = ms_per_call(lambda: up._project_points(coded, one, n1, proj_max_iters=10, c=codes[0]))
    out["four_clouds_ms"] = ms_per_call(lambda: up._project_points(coded, four, n4, proj_max_iters=10, c=codes))
    Pg = 100_000
    small = one[:, :Pg].contiguous()
    per_point = codes[0].expand(Pg, C).contiguous()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        keep_all = UniformProjection(proj_tolerance=1e-30)
        out["generic_100k_ms"] = ms_per_call(lambda: keep_all._project_points(
            coded, small, torch.tensor([Pg], device=dev), proj_max_iters=10, c=per_point), warm=1, rep=3)
    out["one_code_over_uncoded"] = round(out["one_code_ms"] / out["uncoded_ms"], 4)
    out["four_clouds_over_uncoded"] = round(out["four_clouds_ms"] / out["uncoded_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
