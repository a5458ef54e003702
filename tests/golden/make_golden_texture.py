"""Golden vectors of the reference's texture network: its own RenderingNetwork (DSS/models/common.py:313-366) fed by its
own NeuralTexture.forward (DSS/core/texture.py:130-162), which builds the rows [normal, point, embed(normalize(point -
camera centre))] from a point-cloud container and a camera object.  Both containers are stand-ins here that hold plain
tensors and answer exactly the calls NeuralTexture makes (points_packed, normals_packed, packed_to_cloud_idx, device,
clone, update_features_; to, get_camera_center); everything between them -- the branch taken, the concatenation order,
gather_batch_to_packed, F.normalize, the embedder, the network -- is the reference's code.

Three small networks (hidden 64, two layers), 300 points in three ragged clouds; point 5 of every network with a view
direction coincides with its cloud's camera centre:
  texture_wn_c8_f4.npz     weight-normed, c_dim 8, [normal, point], 4 frequencies
  texture_c0_f0.npz        plain, no code, [normal, point], the raw direction
  texture_points_only.npz  plain, no code, the point alone (decoder.dim == 3 and not view_dependent)
Stored: the state dict (reference names), points, normals, codes, camera centres, cloud ids, the float32 rows the decoder
was given, the float32 output, and the float64 output of the same module and inputs.

usage:  python tests/golden/make_golden_texture.py     (writes tests/golden/texture_*.npz)
"""
import os as _os
import sys as _sys

_HERE = _os.path.dirname(_os.path.abspath(__file__))
for _p in (_HERE, _os.path.dirname(_os.path.dirname(_HERE))):      # make_golden.py and the repo root (oracle/)
    if _p not in _sys.path:
        _sys.path.insert(0, _p)

import importlib
import warnings

import torch

CLOUDS = (120, 100, 80)


class _Cloud(object):
    def __init__(self, points, normals, cloud):
        self.points, self.normals, self.cloud, self.features = points, normals, cloud, None
        self.device = points.device

    def points_packed(self):
        return self.points

    def normals_packed(self):
        return self.normals

    def packed_to_cloud_idx(self):
        return self.cloud

    def clone(self):
        return _Cloud(self.points, self.normals, self.cloud)

    def update_features_(self, f):
        self.features = f


class _Cameras(object):
    def __init__(self, centres):
        self.centres = centres

    def to(self, device):
        return self

    def get_camera_center(self):
        return self.centres


def gen_texture():
    from make_golden import npz
    warnings.filterwarnings("ignore")
    Cm = importlib.import_module("DSS.models.common")
    # DSS.core.texture alone: the package's __init__ and the two sibling modules it imports names from (lights and the
    # cloud container, neither on NeuralTexture's path) need the absent pytorch3d
    import types
    import DSS
    core = types.ModuleType("DSS.core")
    core.__path__ = [_os.path.join(_os.path.dirname(DSS.__file__), "core")]
    _sys.modules["DSS.core"] = core
    for sib, attr in (("lighting", "DirectionalLights"), ("cloud", "PointClouds3D")):
        mod = types.ModuleType("DSS.core." + sib)
        setattr(mod, attr, type(attr, (object,), {}))
        _sys.modules["DSS.core." + sib] = mod
    Tx = importlib.import_module("DSS.core.texture")
    cases = (("texture_wn_c8_f4.npz", dict(dim=9, c_dim=8, weight_norm=True, num_frequencies=4), True, True, 31),
             ("texture_c0_f0.npz", dict(dim=9, c_dim=0, weight_norm=False, num_frequencies=0), True, True, 32),
             ("texture_points_only.npz", dict(dim=3, c_dim=0, weight_norm=False, num_frequencies=0), False, False, 33))
    for name, kw, view_dependent, with_view, seed in cases:
        torch.manual_seed(seed)
        net = Cm.RenderingNetwork(hidden_size=64, n_layers=2, **kw)
        g = torch.Generator().manual_seed(seed + 100)
        P = sum(CLOUDS)
        pts = torch.rand(P, 3, generator=g) * 2 - 1
        nrm = torch.randn(P, 3, generator=g)
        nrm = nrm / nrm.norm(dim=-1, keepdim=True) * (0.3 + 2.7 * torch.rand(P, 1, generator=g))
        cams = torch.randn(len(CLOUDS), 3, generator=g)
        cams = cams / cams.norm(dim=-1, keepdim=True) * 3.0
        cloud = torch.repeat_interleave(torch.arange(len(CLOUDS)), torch.tensor(CLOUDS))
        codes = torch.randn(P, kw["c_dim"], generator=g) if kw["c_dim"] else None
        if with_view:
            pts[5] = cams[0]

        seen = {}

        def run(dtype):
            m = Cm.RenderingNetwork(hidden_size=64, n_layers=2, **kw)      # (weight_norm modules do not deepcopy)
            m.load_state_dict(net.state_dict())
            m = m.to(dtype)
            hook = m.register_forward_pre_hook(lambda mod, args: seen.__setitem__(dtype, args[0].detach().clone()))
            tex = Tx.NeuralTexture(m, view_dependent=view_dependent)
            cl = _Cloud(pts.to(dtype), nrm.to(dtype), cloud)
            with torch.no_grad():
                out = tex(cl, c=None if codes is None else codes.to(dtype),
                          **({"cameras": _Cameras(cams.to(dtype))} if with_view else {}))
            hook.remove()
            return out.features
        rgb32, rgb64 = run(torch.float32), run(torch.float64)
        sd = {"sd/" + k: v.detach() for k, v in net.state_dict().items()}
        npz(name, hidden=64, n_layers=2, dim=kw["dim"], c_dim=kw["c_dim"], weight_norm=int(kw["weight_norm"]),
            num_frequencies=kw["num_frequencies"], view_dependent=int(view_dependent), with_view=int(with_view),
            points=pts, normals=nrm, codes=codes if codes is not None else torch.zeros(P, 0), cams=cams, cloud=cloud,
            rows=seen[torch.float32], rgb=rgb32, rgb64=rgb64, **sd)


if __name__ == "__main__":
    import make_golden
    make_golden.install_shims()
    make_golden.load_reference_levelset()
    gen_texture()
