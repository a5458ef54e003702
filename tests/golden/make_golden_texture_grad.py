"""Golden gradients of the reference's texture network: for the three networks and inputs of texture_*.npz (written by
make_golden_texture.py), the reference's own RenderingNetwork under its own NeuralTexture.forward and torch autograd in
float64, loss = sum(rgb * G) with a seeded G.  Stored per network in texture_grad_*.npz: G, the gradient of every
parameter under its state-dict name, and of the points, normals and codes.  The containers are the stand-ins of
make_golden_texture.py; the row assembly (the detach of the view direction included) and the network are the reference's.

usage:  python tests/golden/make_golden_texture_grad.py     (writes tests/golden/texture_grad_*.npz)
"""
import os as _os
import sys as _sys

_HERE = _os.path.dirname(_os.path.abspath(__file__))
for _p in (_HERE, _os.path.dirname(_os.path.dirname(_HERE))):
    if _p not in _sys.path:
        _sys.path.insert(0, _p)

import importlib
import types
import warnings

import numpy as np
import torch

NAMES = ("texture_wn_c8_f4.npz", "texture_c0_f0.npz", "texture_points_only.npz")


def gen_texture_grad():
    from make_golden import npz
    from make_golden_texture import _Cameras, _Cloud
    warnings.filterwarnings("ignore")
    Cm = importlib.import_module("DSS.models.common")
    import DSS
    core = types.ModuleType("DSS.core")                       # as make_golden_texture.py: DSS.core.texture alone
    core.__path__ = [_os.path.join(_os.path.dirname(DSS.__file__), "core")]
    _sys.modules["DSS.core"] = core
    for sib, attr in (("lighting", "DirectionalLights"), ("cloud", "PointClouds3D")):
        mod = types.ModuleType("DSS.core." + sib)
        setattr(mod, attr, type(attr, (object,), {}))
        _sys.modules["DSS.core." + sib] = mod
    Tx = importlib.import_module("DSS.core.texture")
    for k, name in enumerate(NAMES):
        z = np.load(_os.path.join(_HERE, name))
        kw = dict(dim=int(z["dim"]), c_dim=int(z["c_dim"]), weight_norm=bool(z["weight_norm"]),
                  num_frequencies=int(z["num_frequencies"]))
        m = Cm.RenderingNetwork(hidden_size=int(z["hidden"]), n_layers=int(z["n_layers"]), **kw)
        m.load_state_dict({f[3:]: torch.from_numpy(z[f]) for f in z.files if f.startswith("sd/")}, strict=True)
        m = m.double()
        pts = torch.from_numpy(z["points"]).double().requires_grad_(True)
        nrm = torch.from_numpy(z["normals"]).double().requires_grad_(True)
        codes = torch.from_numpy(z["codes"]).double().requires_grad_(True) if kw["c_dim"] else None
        cams = torch.from_numpy(z["cams"]).double()
        cloud = torch.from_numpy(z["cloud"])
        G = torch.randn(pts.shape[0], 3, generator=torch.Generator().manual_seed(700 + k), dtype=torch.float64)
        tex = Tx.NeuralTexture(m, view_dependent=bool(z["view_dependent"]))
        out = tex(_Cloud(pts, nrm, cloud), c=codes, **({"cameras": _Cameras(cams)} if bool(z["with_view"]) else {}))
        (out.features * G).sum().backward()
        grads = {"grad/" + n: p.grad for n, p in m.named_parameters()}
        npz("texture_grad_" + name[len("texture_"):], G=G, grad_points=pts.grad,
            grad_normals=nrm.grad if nrm.grad is not None else torch.zeros(0, 3, dtype=torch.float64),
            grad_codes=codes.grad if codes is not None else torch.zeros(pts.shape[0], 0, dtype=torch.float64), **grads)


if __name__ == "__main__":
    import make_golden
    make_golden.install_shims()
    make_golden.load_reference_levelset()
    gen_texture_grad()
