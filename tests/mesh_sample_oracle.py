"""The draw of include/isopoints.h section I restated in numpy, and the meshes the sampling tests share.  No GPU, no
library: tests/test_mesh_sample_cpu.py checks this file against iso_mesh_sample_draw and on its own statistics,
tests/test_mesh_sample_gpu.py checks the kernels against it."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> the four output words, uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def seed_of(k):
    """The int64 seed sample_points_from_meshes draws from torch.Generator().manual_seed(k)."""
    import torch
    return int(torch.empty((), dtype=torch.int64).random_(generator=torch.Generator().manual_seed(k)))


def draw_words(seed, mesh, samples):
    """r0..r3 of the samples `samples` (array) of mesh `mesh` under `seed` (any int64, taken as its 64 bits)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = np.asarray(samples, dtype=np.uint64)
    return philox4x32_10((s & np.uint64(MASK), s >> np.uint64(32), np.uint64(int(mesh) & MASK), np.uint64(0)),
                         (seed & MASK, seed >> 32))


def uniforms(seed, mesh, samples):
    """uf (float64), u, v (float32): exact conversions of the four words."""
    r0, r1, r2, r3 = draw_words(seed, mesh, samples)
    k = (r0.astype(np.uint64) << np.uint64(21)) | (r1.astype(np.uint64) >> np.uint64(11))
    uf = k.astype(np.float64) * 2.0 ** -53
    u = (r2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    v = (r3 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return uf, u, v


def face_areas32(tris):
    """float32 areas of (F,3,3) float32 triangles, in the order of operations of the header."""
    t = np.asarray(tris, dtype=np.float32)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    mx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    my = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    mz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return (np.float32(0.5) * np.sqrt((mx * mx + my * my) + mz * mz)).astype(np.float32)


def bary32(u, v):
    s = np.sqrt(u.astype(np.float32))
    one = np.float32(1.0)
    return np.stack([one - s, s * (one - v), s * v], axis=1).astype(np.float32)


def sample(tris, seed, mesh, S, areas=None):
    """The oracle's draw on one mesh: dict(face (S,) local index or -1, bary (S,3) f32, t (S,), C (F,), A, margin (S,) =
    the distance of t to the nearest boundary of C)."""
    areas = face_areas32(tris) if areas is None else np.asarray(areas, dtype=np.float32)
    C = np.cumsum(areas.astype(np.float64))
    A = float(C[-1]) if len(C) else 0.0
    if not A > 0.0:
        return dict(face=np.full(S, -1, dtype=np.int64), bary=np.zeros((S, 3), np.float32), t=np.zeros(S), C=C, A=A,
                    margin=np.full(S, np.inf))
    uf, u, v = uniforms(seed, mesh, np.arange(S))
    t = uf * A
    face = np.searchsorted(C, t, side="right")          # the first f with C[f] > t
    assert face.max() < len(C)
    below = np.where(face > 0, C[np.maximum(face - 1, 0)], -np.inf)
    margin = np.minimum(C[face] - t, t - below)
    return dict(face=face.astype(np.int64), bary=bary32(u, v), t=t, C=C, A=A, margin=margin)


# ------------------------------------------------------------------------------------------------------------ the meshes
def icosphere(level):
    """(verts (V,3) float64, faces (F,3) int64) of the unit icosphere after `level` subdivisions: 20 * 4^level faces."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
         [9, 8, 1]]
    verts = [x / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, faces = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            faces += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = faces
    return np.stack(verts), np.array(f, dtype=np.int64)


_CACHE = {}


def scaled_icosphere():
    """Level 2 = 320 faces, scaled by (3, 1, 0.5) so that the areas differ: (verts (162,3) f32, faces (320,3) int64)."""
    if "ico" not in _CACHE:
        v, f = icosphere(2)
        _CACHE["ico"] = ((v * np.array([3.0, 1.0, 0.5])).astype(np.float32), f)
    return _CACHE["ico"]


def warped_grid(n=200):
    """An n x n grid of quads on [0, 1]^2, lifted and sheared so that no two faces have the same area, two triangles per
    quad: (verts ((n+1)^2, 3) f32, faces (2 n^2, 3) int64)."""
    if ("grid", n) not in _CACHE:
        x, y = np.meshgrid(np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1), indexing="ij")
        xs = x + 0.3 * x * x
        ys = y + 0.2 * np.sin(3.0 * x) * y
        z = 0.25 * np.sin(5.0 * x) * np.cos(4.0 * y)
        verts = np.stack([xs, ys, z], axis=-1).reshape(-1, 3).astype(np.float32)
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
        faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
        _CACHE[("grid", n)] = (verts, faces.astype(np.int64))
    return _CACHE[("grid", n)]


def wide_range_mesh():
    """1 001 faces with vertices of their own: face 500 has area 0.5 * 1.4 * 1.5 ~ 1, the others are right triangles with
    legs of 1.2e-4 .. 1.6e-4 (area ~ 1e-8) spread along x: (verts (3003,3) f32, faces (1001,3) int64)."""
    if "wide" not in _CACHE:
        rng = np.random.RandomState(5)
        F = 1001
        org = np.stack([np.linspace(-2.0, 2.0, F), rng.uniform(-1, 1, F), rng.uniform(-1, 1, F)], axis=1)
        legs = rng.uniform(1.2e-4, 1.6e-4, (F, 2))
        legs[500] = (1.4, 1.5)
        tris = np.stack([org, org + np.stack([legs[:, 0], 0 * legs[:, 0], 0 * legs[:, 0]], 1),
                         org + np.stack([0 * legs[:, 1], legs[:, 1], 0.3 * legs[:, 1]], 1)], axis=1)
        _CACHE["wide"] = (tris.reshape(-1, 3).astype(np.float32), np.arange(3 * F, dtype=np.int64).reshape(F, 3))
    return _CACHE["wide"]


def chi_square(face, areas, S):
    """Pearson's statistic of the face counts against S * area / A."""
    areas = np.asarray(areas, dtype=np.float64)
    expect = S * areas / areas.sum()
    count = np.bincount(face, minlength=len(areas)).astype(np.float64)
    return float(((count - expect) ** 2 / expect).sum())


CHI2_BOUND = 319 + 6 * math.sqrt(2 * 319)        # 320 faces: mean 319, sd sqrt(638) = 25.3; six of them above: 470.6


def bary_mean_bound(S):
    """Each weight of a uniform point of a triangle has mean 1/3 and variance 1/18: five standard errors."""
    return 5.0 * math.sqrt(1.0 / 18.0 / S)
