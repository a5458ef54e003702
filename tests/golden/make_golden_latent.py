"""Golden vectors of the reference's latent-conditioned SIREN: its own Siren(c_dim = 32) class
(DSS/models/common.py:90-165; the code is concatenated in front of the point, [c, x], :150-152)
evaluated through the reference's _compute_sdf_and_grad / _project_points (levelset_sampling.py:142-170,
:290-351) with a per-point code c of shape (P, C) -- the reference's projection loop passes `c` to
model.forward on the points it evaluates, so a per-point code and ONE chunk (max_points_per_pass >= P)
with a stopping tolerance no point meets (1e-30: every point stays active) keep codes and points aligned.

Two networks (3 -> 256 x 3 -> 1 and 3 -> 128 x 2 -> 1, code width 32), 3 codes, 1500 points in three
ragged clouds.  Stored: the state dict (reference names, net.<i>.linear.* / net.<L+1>.*), the codes, the
points and their cloud ids, the forward value, the gradient with respect to the coordinates (float32 and
float64 autograd), and the points / normals after 4 Newton moves of the reference's loop.

usage:  python tests/golden/make_golden_latent.py     (writes tests/golden/siren_latent_*.npz)
"""
import os as _os
import sys as _sys

_HERE = _os.path.dirname(_os.path.abspath(__file__))
for _p in (_HERE, _os.path.dirname(_os.path.dirname(_HERE))):      # make_golden.py and the repo root (oracle/)
    if _p not in _sys.path:
        _sys.path.insert(0, _p)

import copy
import importlib
import warnings

import torch

C_DIM = 32
CLOUDS = (700, 500, 300)
T = 4


def gen_latent(L):
    from make_golden import npz
    warnings.filterwarnings("ignore")
    Cm = importlib.import_module("DSS.models.common")
    for name, H, NL, seed in (("siren_latent_256x3.npz", 256, 3, 21), ("siren_latent_128x2.npz", 128, 2, 22)):
        torch.manual_seed(seed)
        m = Cm.Siren(dim=3, hidden_size=H, n_layers=NL, c_dim=C_DIM, first_omega_0=30, hidden_omega_0=30.0)
        g = torch.Generator().manual_seed(seed + 100)
        codes = torch.randn(len(CLOUDS), C_DIM, generator=g)
        P = sum(CLOUDS)
        x = (torch.rand(P, 3, generator=g) - 0.5) * 1.6
        cloud = torch.repeat_interleave(torch.arange(len(CLOUDS)), torch.tensor(CLOUDS))
        c_pt = codes[cloud]                                                   # (P, C): the code of every point
        up = L.UniformProjection(max_points_per_pass=P)
        sdf, grad = up._compute_sdf_and_grad(x.clone(), m, c=c_pt)
        # float64 autograd of the same module
        m64 = copy.deepcopy(m).double()
        x64 = x.double().requires_grad_(True)
        f64 = m64(x64, c=c_pt.double()).sdf
        (g64,) = torch.autograd.grad([f64], [x64], torch.ones_like(f64))
        res = up._project_points(m, x.clone().unsqueeze(0), torch.tensor([P]), proj_max_iters=T, proj_tolerance=1e-30,
                                 c=c_pt)
        sd = {"sd/" + k: v.detach() for k, v in m.state_dict().items()}
        npz(name, hidden=H, n_layers=NL, c_dim=C_DIM, codes=codes, points=x, cloud=cloud, sdf=sdf, grad=grad,
            sdf64=f64.detach().reshape(-1), grad64=g64, T=T, fixed_points=res.points[0], fixed_normals=res.normals[0],
            **sd)


if __name__ == "__main__":
    import make_golden
    make_golden.install_shims()
    gen_latent(make_golden.load_reference_levelset())
