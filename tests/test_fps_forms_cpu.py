"""Farthest-point sampling without a GPU: the dispatch of iso_farthest_point_sampling on both sides of every boundary
(iso_farthest_point_sampling_form), the guard that the shapes of tests/test_fps_forms_gpu.py reach every FPS kernel of the
built library, and the oracle itself against the definition."""
import os
import re

import numpy as np
import pytest
import torch

from test_fps_forms_gpu import FORMS, NO_COOP, ONE_WG
from util import FPS_F64_SLACK, fps_float64_deficit, sphere_cloud

REG, LAZY, GRID, WALK = 100, 200, 300, 0


def _form(p, monkeypatch=None, env=None):
    from iso_points_amd import _lib
    if env:
        monkeypatch.setenv(env, "1")
    try:
        return _lib.load().iso_farthest_point_sampling_form(p, 0)
    finally:
        if env:
            monkeypatch.delenv(env)


# (last stride of a form, its code); the next stride takes the next entry's form
DEFAULT_RANGES = [(1024, REG + 1), (2048, REG + 2), (4095, REG + 4), (131072, LAZY + 1), (262144, LAZY + 2),
                  (524288, LAZY + 4), (1048576, LAZY + 8), (2097152, LAZY + 16), (4194304, GRID + 16), (2 ** 31 - 1, WALK)]
NO_COOP_RANGES = [(1024, REG + 1), (2048, REG + 2), (4096, REG + 4), (8192, REG + 8), (2 ** 31 - 1, WALK)]


def _both_sides(ranges):
    out, first = [], 1
    for last, code in ranges:
        out += [(first, code), (last, code)]
        first = last + 1
    return out


@pytest.mark.parametrize("p,code", _both_sides(DEFAULT_RANGES))
def test_dispatch_boundaries(p, code):
    assert os.environ.get(NO_COOP) is None and os.environ.get(ONE_WG) is None
    assert _form(p) == code


@pytest.mark.parametrize("p,code", _both_sides(NO_COOP_RANGES))
def test_dispatch_boundaries_without_cooperative_launch(p, code, monkeypatch):
    """ISO_FPS_NO_COOPERATIVE: as if the first cooperative launch had been refused -- registers up to 8 192, k_fps above."""
    assert _form(p, monkeypatch, NO_COOP) == code
    assert _form(p) == [c for last, c in DEFAULT_RANGES if p <= last][0]      # read on every call: gone again


@pytest.mark.parametrize("p", [p for p, _ in _both_sides(DEFAULT_RANGES)])
def test_dispatch_one_workgroup_switch(p, monkeypatch):
    assert _form(p, monkeypatch, ONE_WG) == WALK
    monkeypatch.setenv(NO_COOP, "1")
    assert _form(p, monkeypatch, ONE_WG) == WALK


def test_dispatch_refuses_strides_outside_the_contract():
    assert _form(0) == -1 and _form(-3) == -1 and _form(2 ** 31) == -1


def _kernel_of(code):
    return "k_fps" if code == WALK else "%s<%d>" % ({1: "k_fps_reg", 2: "k_fps_lazy", 3: "k_fps_grid"}[code // 100], code % 100)


def test_gpu_shapes_reach_every_fps_kernel_of_the_library(monkeypatch):
    """The orphan guard: FORMS (the shapes tests/test_fps_forms_gpu.py launches) taken through the form function reach
    exactly the FPS kernels the code object holds.  A re-dispatch that orphans an instance, or a new instance without a
    shape, fails here, on the CPU."""
    from test_abi import _code_object_kernels
    in_library = set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_fps[a-z_]*)(?:ILi(\d+)E)?E", name)
        if m and len(m.group(2)) == int(m.group(1)):
            in_library.add(m.group(2) + ("<%s>" % m.group(3) if m.group(3) else ""))
    reached = set()
    for p, env, code in FORMS:
        assert _form(p, monkeypatch, env) == code, (p, env)
        reached.add(_kernel_of(code))
    assert len(in_library) == 11, sorted(in_library)
    assert reached == in_library, (sorted(reached - in_library), sorted(in_library - reached))


# ---- the oracle itself ----------------------------------------------------------------------------------------------------
def _oracle_clouds():
    base = sphere_cloud(3000, seed=9)[0]
    lat = torch.stack(torch.meshgrid(*([torch.arange(14.0)] * 3), indexing="ij"), -1).view(-1, 3) * 0.1
    return {"sphere": base, "lattice": lat, "offset_100": 100.0 + 1e-3 * base, "scaled_1e-18": base * 1e-18}


@pytest.mark.parametrize("name", ["sphere", "lattice", "offset_100", "scaled_1e-18"])
def test_oracle_sequence_is_farthest_in_float64(name):
    """oracle.farthest_point_sampling against the float64 statement of the definition (util.fps_float64_deficit): every
    chosen point's float64 min-distance is within 2^-20 relative of the float64 maximum (four f32 roundings are 2^-22), and 0
    where the maximum is 0.  300 samples: on the scaled cloud the min-distances stay above 1e-38, where an f32 rounding is
    still relative (a denormal's is absolute, and no relative bound holds for it)."""
    from oracle import iso_oracle as O
    cloud = _oracle_clouds()[name]
    seq = O.farthest_point_sampling(cloud, 300, start=4)
    assert seq[0] == 4 and len(set(seq.tolist())) == 300
    deficit = fps_float64_deficit(cloud, seq)
    print("%s: worst float64 deficit %.3g" % (name, deficit))
    assert deficit <= FPS_F64_SLACK


def test_oracle_tie_rule_against_a_plain_loop():
    """The oracle's arg-max against ten lines of Python with the rule spelled out: a later point replaces the best only when
    strictly farther, so the lowest index wins a tie -- 200 points, 60 of them copies of others, sampled past exhaustion."""
    from oracle import iso_oracle as O
    p = sphere_cloud(200, seed=3)[0]
    p[140:] = p[:60]
    q = p.numpy()
    mind, cur, seq = [np.float32(np.finfo(np.float32).max)] * 200, 7, []
    for _ in range(180):
        seq.append(cur)
        best = -1
        for i in range(200):
            d = q[i] - q[cur]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            mind[i] = min(mind[i], d2)
            if best < 0 or mind[i] > mind[best]:
                best = i
        cur = best
    assert O.farthest_point_sampling(p, 180, start=7).tolist() == seq
    assert seq[140:] == [0] * 40                            # 140 distinct points: then every distance is 0
