"""The elimination of include/isopoints.h section L restated in numpy: brute force, no grid, no GPU, no library.
tests/test_even_sample_cpu.py checks this file on its own (serial == rounds), tests/test_even_sample_gpu.py checks the
kernels against it on the bits the GPU was given."""
import numpy as np

UNDECIDED, KEEP, REMOVED = 0, 1, 2


def conflicts(points_f32, r):
    """(P,P) bool: d2(i, j) <= r2 with d2 = (dx*dx + dy*dy) + dz*dz and r2 = r * r, every operation rounded to float32 (numpy
    does not contract).  The diagonal is True; callers only ever look below it."""
    p = np.asarray(points_f32, dtype=np.float32)
    r = np.float32(r)
    r2 = np.float32(r * r)
    sq = []
    for c in range(3):
        d = p[:, None, c] - p[None, :, c]
        sq.append(d * d)
    d2 = (sq[0] + sq[1]) + sq[2]
    assert d2.dtype == np.float32
    return d2 <= r2


def _entry_state(P, length, valid):
    length = P if length is None else int(length)
    state = np.full(P, REMOVED, dtype=np.uint8)
    ok = np.arange(P) < length
    if valid is not None:
        ok &= np.asarray(valid).astype(bool)
    state[ok] = UNDECIDED
    return state


def _result(state):
    mask = state == KEEP
    P = len(state)
    sel = np.full(P, -1, dtype=np.int64)
    idx = np.nonzero(mask)[0]
    sel[: len(idx)] = idx
    return mask, sel, int(len(idx))


def serial(points_f32, r, length=None, valid=None, conf=None):
    """Serial dart throwing in index order on one cloud (P,3): (mask (P,) bool, sel (P,) int64 ascending kept indices then
    -1, kept).  `conf` takes a conflicts() matrix that is already there."""
    conf = conflicts(points_f32, r) if conf is None else conf
    state = _entry_state(len(conf), length, valid)
    kept = np.zeros(len(conf), dtype=bool)
    for s in range(len(conf)):
        if state[s] != UNDECIDED:
            continue
        if (conf[s, :s] & kept[:s]).any():
            state[s] = REMOVED
        else:
            state[s] = KEEP
            kept[s] = True
    return _result(state)


def rounds(points_f32, r, length=None, valid=None, conf=None):
    """The parallel form with synchronous sweeps (every sample of a round reads the states the previous round left):
    (mask, sel, kept, number of rounds until nothing is UNDECIDED)."""
    conf = conflicts(points_f32, r) if conf is None else conf
    P = len(conf)
    below = np.tril(conf, k=-1)                       # below[s, j]: j < s and they conflict
    state = _entry_state(P, length, valid)
    n = 0
    while (state == UNDECIDED).any():
        keep_below = (below & (state == KEEP)[None, :]).any(axis=1)
        open_below = (below & (state == UNDECIDED)[None, :]).any(axis=1)
        und = state == UNDECIDED
        new = state.copy()
        new[und & keep_below] = REMOVED
        new[und & ~keep_below & ~open_below] = KEEP
        state = new
        n += 1
    return _result(state) + (n,)


def sphere_cloud(P, seed):
    """P float32 points on the unit sphere, uniform."""
    v = np.random.RandomState(seed).randn(P, 3)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def chain(n, r, shuffle_seed=None):
    """n collinear float32 points at spacing 0.6 r along x, in index order, or with the indices shuffled by a fixed
    permutation: (points, order) with points[k] = the chain's position order[k]."""
    order = np.arange(n) if shuffle_seed is None else np.random.RandomState(shuffle_seed).permutation(n)
    pts = np.zeros((n, 3), dtype=np.float32)
    pts[:, 0] = (order.astype(np.float64) * 0.6 * float(np.float32(r))).astype(np.float32)
    return pts, order


# (mesh, S) of the sampler cases the CPU and the GPU tests share
SAMPLER_CASES = (("ico2", 300), ("ico3", 1000), ("scaled", 500))


def sampler_mesh(name):
    """(verts (V,3) float32, faces (F,3) int64): icosphere(2), icosphere(3) or the scaled icosphere."""
    import mesh_sample_oracle as M
    if name == "scaled":
        return M.scaled_icosphere()
    v, f = M.icosphere(int(name[-1]))
    return v.astype(np.float32), f


def default_radius(verts, faces, S):
    """sqrt(A / (3 S)) with A the float64 sum of the float32 face areas, as float32: the default of
    sample_points_from_meshes_even."""
    import mesh_sample_oracle as M
    A = float(np.sum(M.face_areas32(np.asarray(verts, dtype=np.float32)[faces]).astype(np.float64)))
    return np.float32(np.sqrt(A / (3.0 * S)))


def oracle_draw_points(verts, faces, seed, S):
    """The float32 points and the local faces of the sampler oracle's first S draws on one mesh: (w0 v0 + w1 v1) + w2 v2 per
    component in float32."""
    import mesh_sample_oracle as M
    tris = np.asarray(verts, dtype=np.float32)[faces]
    d = M.sample(tris, seed, 0, S)
    t, w = tris[d["face"]], d["bary"]
    pts = ((w[:, 0:1] * t[:, 0] + w[:, 1:2] * t[:, 1]).astype(np.float32) + w[:, 2:3] * t[:, 2]).astype(np.float32)
    return pts, d["face"]
