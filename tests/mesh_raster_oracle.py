"""numpy oracle of the mesh rasteriser (include/isopoints.h section M): brute force over all (pixel, face) pairs, the rule
in float64, and the same rule statement for statement in float32 (the "f32 restatement", which the kernel of
csrc/mesh_raster.hip follows operation for operation).

Both start from the same inputs: the float32 face vertices and the float32 pixel centres X = 1 - (2c+1)/S.

Safe pixels.  Per pair T is the largest of the four sums |a| + |b| of the two products of an edge function (three edges
and the area), and tol = 16 * 2^-24 * T / |area|: an edge function carries at most about four roundings relative to T, the
quotient adds the area's share, 16 leaves a factor of two.  A pixel is UNSAFE if some non-skipped face has |w_i| <= tol
(float32 cannot decide the side) or if two of its K + 1 nearest candidates have depths closer than 1e-5 relative without
being equal (equal depths are safe: the tie rule decides them).  pix_to_face is compared exactly on every safe pixel."""
import functools
import math

import numpy as np

AREA_EPS = 1e-8
SEG_EPS = 1e-8
DEPTH_REL = 1e-5
UNSAFE_CAP = 0.01


def pixel_centres(S):
    """float32 centres of output columns (= rows) 0 .. S-1."""
    i = np.arange(S)
    return np.float32(1.0) - (2 * i + 1).astype(np.float32) / np.float32(S)


def _seg_dist2(px, py, ax, ay, bx, by, dt):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    short = l2 <= dt(SEG_EPS)
    qx, qy = px - bx, py - by
    d_end = qx * qx + qy * qy
    t = (dx * (px - ax) + dy * (py - ay)) / np.where(short, dt(1.0), l2)
    t = np.minimum(np.maximum(t, dt(0.0)), dt(1.0))
    qx, qy = px - (ax + t * dx), py - (ay + t * dy)
    return np.where(short, d_end, qx * qx + qy * qy)


def rasterize(face_verts, first, num, S, K, perspective_correct=False, cull_backfaces=False, dtype=np.float64):
    """face_verts (F,3,3) float32, first / num (N,) -> dict(pix_to_face (N,S,S,K) int64, zbuf, bary (N,S,S,K,3), dists,
    unsafe (N,S,S) bool, covered (N,S,S) bool), values in `dtype`.  unsafe is computed in float64 whatever dtype is."""
    dt = np.dtype(dtype).type
    fv32 = np.asarray(face_verts, dtype=np.float32).reshape(-1, 3, 3)
    first, num = np.asarray(first).astype(np.int64), np.asarray(num).astype(np.int64)
    N = len(first)
    cen = pixel_centres(S)
    py, px = [a.reshape(-1, 1) for a in np.meshgrid(cen, cen, indexing="ij")]          # (P,1): row-major pixels
    p2f = np.full((N, S * S, K), -1, dtype=np.int64)
    zbuf = np.full((N, S * S, K), -1.0, dtype=dt)
    bary = np.full((N, S * S, K, 3), -1.0, dtype=dt)
    dists = np.full((N, S * S, K), -1.0, dtype=dt)
    unsafe = np.zeros((N, S * S), dtype=bool)
    with np.errstate(all="ignore"):
        for n in range(N):
            f0, fn = int(first[n]), int(num[n])
            if fn == 0:
                continue
            v32 = fv32[f0:f0 + fn]
            res = _one_mesh(v32.astype(dt), px.astype(dt), py.astype(dt), K, perspective_correct, cull_backfaces, dt)
            ids, z, b, d = res
            hit = ids >= 0
            p2f[n] = np.where(hit, ids + f0, -1)
            zbuf[n], bary[n], dists[n] = z, b, d
            unsafe[n] = _unsafe(v32.astype(np.float64), px.astype(np.float64), py.astype(np.float64), K, perspective_correct,
                                cull_backfaces)
    shape = (N, S, S)
    return dict(pix_to_face=p2f.reshape(shape + (K,)), zbuf=zbuf.reshape(shape + (K,)), bary=bary.reshape(shape + (K, 3)),
                dists=dists.reshape(shape + (K,)), unsafe=unsafe.reshape(shape), covered=(p2f[..., 0] >= 0).reshape(shape))


def _pairs(v, px, py, perspective_correct, cull_backfaces, dt):
    """All pairs of one mesh: valid (P,F), pz, (b0, b1, b2), (w0, w1, w2), skip (F,), area (F,), the edge products."""
    x0, y0, z0 = v[:, 0, 0][None], v[:, 0, 1][None], v[:, 0, 2][None]
    x1, y1, z1 = v[:, 1, 0][None], v[:, 1, 1][None], v[:, 1, 2][None]
    x2, y2, z2 = v[:, 2, 0][None], v[:, 2, 1][None], v[:, 2, 2][None]
    a_p, a_q = (x2 - x0) * (y1 - y0), (y2 - y0) * (x1 - x0)
    area = a_p - a_q
    finite = np.isfinite(v.reshape(len(v), 9)).all(axis=1)[None]
    skip = ~finite | ~(np.abs(area) > dt(AREA_EPS)) | (np.maximum(np.maximum(z0, z1), z2) < 0)
    if cull_backfaces:
        skip = skip | (area < 0)
    e0p, e0q = (px - x1) * (y2 - y1), (py - y1) * (x2 - x1)            # edge(v1, v2; p)
    e1p, e1q = (px - x2) * (y0 - y2), (py - y2) * (x0 - x2)            # edge(v2, v0; p)
    e2p, e2q = (px - x0) * (y1 - y0), (py - y0) * (x1 - x0)            # edge(v0, v1; p)
    w0, w1, w2 = (e0p - e0q) / area, (e1p - e1q) / area, (e2p - e2q) / area
    inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
    b0, b1, b2 = w0, w1, w2
    if perspective_correct:
        t0, t1, t2 = w0 * z1 * z2, w1 * z0 * z2, w2 * z0 * z1
        den = (t0 + t1) + t2
        b0, b1, b2 = t0 / den, t1 / den, t2 / den
    pz = (b0 * z0 + b1 * z1) + b2 * z2
    valid = inside & ~skip & (pz >= 0) & np.isfinite(pz)
    prods = (a_p, a_q, e0p, e0q, e1p, e1q, e2p, e2q)
    return valid, pz, (b0, b1, b2), (w0, w1, w2), skip, area, prods


def _one_mesh(v, px, py, K, perspective_correct, cull_backfaces, dt):
    valid, pz, b, _, _, _, _ = _pairs(v, px, py, perspective_correct, cull_backfaces, dt)
    P, F = valid.shape
    key = np.where(valid, pz + dt(0.0), dt(np.inf))
    order = np.argsort(key, axis=1, kind="stable")[:, :K]             # ties: the lower face index (faces are in index order)
    if order.shape[1] < K:
        order = np.concatenate([order, np.zeros((P, K - order.shape[1]), dtype=order.dtype)], axis=1)
        got = np.concatenate([np.take_along_axis(valid, order[:, :F], axis=1), np.zeros((P, K - F), dtype=bool)], axis=1)
    else:
        got = np.take_along_axis(valid, order, axis=1)
    ids = np.where(got, order, -1)
    take = lambda a: np.take_along_axis(np.broadcast_to(a, (P, F)), np.minimum(order, F - 1), axis=1)
    z = np.where(got, take(pz), dt(-1.0))
    bb = np.stack([np.where(got, take(c), dt(-1.0)) for c in b], axis=-1)
    x0, y0, x1, y1, x2, y2 = [take(v[:, i, j][None]) for i, j in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))]
    d = np.minimum(np.minimum(_seg_dist2(px, py, x0, y0, x1, y1, dt), _seg_dist2(px, py, x0, y0, x2, y2, dt)),
                   _seg_dist2(px, py, x1, y1, x2, y2, dt))
    return ids, z, bb, np.where(got, -d, dt(-1.0))


def _unsafe(v, px, py, K, perspective_correct, cull_backfaces):
    dt = np.float64
    valid, pz, _, w, skip, area, prods = _pairs(v, px, py, perspective_correct, cull_backfaces, dt)
    T = np.zeros(np.broadcast(prods[2], prods[0]).shape)
    for a, b in zip(prods[0::2], prods[1::2]):
        T = np.maximum(T, np.abs(a) + np.abs(b))
    tol = 16.0 * 2.0 ** -24 * T / np.abs(area)
    near_edge = np.zeros(T.shape, dtype=bool)
    for wi in w:
        near_edge |= np.abs(wi) <= tol
    out = (near_edge & ~skip).any(axis=1)
    key = np.sort(np.where(valid, pz, np.inf), axis=1)[:, :K + 1]
    if key.shape[1] > 1:
        lo, hi = key[:, :-1], key[:, 1:]
        both = np.isfinite(lo) & np.isfinite(hi)
        close = both & (hi != lo) & (np.where(both, hi - lo, 1.0) <= DEPTH_REL * np.where(both, np.maximum(np.abs(hi), np.abs(lo)), 1.0))
        out |= close.any(axis=1)
    return out


def half_step(top):
    return 0.5 * 2.0 ** (math.floor(math.log2(top)) - 23) if top > 0 else 0.0


def bounds(r64, r32):
    """A per output: 4 x the largest error of the float32 restatement against float64 on the slots of safe pixels whose
    face agrees, the error taken as at least half a float32 step at the largest reference entry -> ({name: A}, {name: err})."""
    same = (r64["pix_to_face"] == r32["pix_to_face"]) & (r64["pix_to_face"] >= 0) & ~r64["unsafe"][..., None]
    A, errs = {}, {}
    for name in ("zbuf", "bary", "dists"):
        m = same[..., None] if name == "bary" else same
        m = np.broadcast_to(m, r64[name].shape)
        ref, got = r64[name][m], r32[name][m].astype(np.float64)
        err = float(np.abs(got - ref).max()) if ref.size else 0.0
        top = float(np.abs(ref).max()) if ref.size else 0.0
        A[name], errs[name] = 4.0 * max(err, half_step(top)), err
    return A, errs


# ------------------------------------------------------------------------------------------------------------ scenes
class PackedMeshes:
    """The four accessors of a pytorch3d Meshes that rasterize_meshes reads, over packed face vertices (F,3,3): every face
    gets its own three vertices."""

    def __init__(self, face_verts, first, num, device="cpu"):
        import torch
        fv = torch.as_tensor(np.asarray(face_verts, dtype=np.float32)).reshape(-1, 3, 3)
        self._verts = fv.reshape(-1, 3).to(device)
        self._faces = torch.arange(fv.shape[0] * 3, dtype=torch.int64).reshape(-1, 3).to(device)
        self._first = torch.as_tensor(np.asarray(first, dtype=np.int64)).to(device)
        self._num = torch.as_tensor(np.asarray(num, dtype=np.int64)).to(device)

    def verts_packed(self):
        return self._verts

    def faces_packed(self):
        return self._faces

    def mesh_to_faces_packed_first_idx(self):
        return self._first

    def num_faces_per_mesh(self):
        return self._num


def edge_scene():
    """Faces against the image's border and the tile grid: one covering the whole image, one with vertices 1e4 away that
    covers it too, one partly and one wholly off-screen, a small one in the middle (their coordinates are no round
    decimals: with round ones their edge lines run exactly through pixel centres at S = 15 and 50, which are unsafe by
    definition).  -> face_verts (5,3,3) float32."""
    return np.array([[[3.0, -3.0, 5.0], [-3.0, -3.0, 5.0], [0.0, 4.0, 5.0]],
                     [[1e4, -1e4, 3.0], [-1e4, -1e4, 3.5], [0.0, 1e4, 4.0]],
                     [[1.5311, 0.2113, 2.0], [0.6137, -0.4271, 2.5], [0.7219, 0.9341, 1.5]],
                     [[3.0, 3.0, 1.0], [2.0, 3.0, 1.0], [2.5, 2.0, 1.0]],
                     [[0.3137, -0.2071, 1.0], [-0.2913, -0.2539, 1.2], [0.0517, 0.4177, 0.8]]], dtype=np.float32)


def skip_scene():
    """A background face and the faces the rule skips: zero area, every z < 0, a NaN vertex; and one whose interpolated
    depth is negative over part of its pixels (kept where pz >= 0).  -> face_verts (5,3,3) float32."""
    return np.array([[[0.9, -0.9, 4.0], [-0.9, -0.9, 4.0], [0.0, 0.9, 4.0]],
                     [[0.5, 0.5, 1.0], [0.0, 0.0, 1.0], [-0.5, -0.5, 1.0]],
                     [[0.6, -0.6, -1.0], [-0.6, -0.6, -2.0], [0.0, 0.6, -0.5]],
                     [[0.6, -0.6, 1.0], [np.nan, -0.6, 1.0], [0.0, 0.6, 1.0]],
                     [[0.7, -0.5, -1.0], [-0.7, -0.5, 2.0], [0.0, 0.7, 2.0]]], dtype=np.float32)


def icosphere(level):
    import mesh_sample_oracle as M
    v, f = M.icosphere(level)
    return v.astype(np.float32), f


def look_at_projection(dist=2.7, elev=20.0, azim=30.0, fov=60.0):
    """(view, proj) float32 numpy (4,4): iso_points_amd.cameras.look_at_view / perspective, proj the full world -> NDC."""
    from iso_points_amd import cameras
    V = cameras.look_at_view(dist, elev, azim)
    return V.numpy().astype(np.float32), (V @ cameras.perspective(fov)).numpy().astype(np.float32)


def to_ndc(verts, view, proj):
    """pytorch3d's transform in float32 numpy: x, y from [v, 1] @ proj with the homogeneous divide, z from [v, 1] @ view."""
    hom = np.concatenate([verts.astype(np.float32), np.ones((len(verts), 1), dtype=np.float32)], axis=1)
    pn, pv = hom @ proj, hom @ view
    return np.concatenate([pn[:, :2] / pn[:, 3:4], pv[:, 2:3]], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_faces(level):
    """(face_verts (F,3,3) float32 in NDC with view z, world face verts (F,3,3) float32) of the camera of the tests."""
    v, f = icosphere(level)
    view, proj = look_at_projection()
    return to_ndc(v, view, proj)[f], v[f]


SPHERE_CASES = [(level, S, persp) for level in (2, 3) for S in (48, 33) for persp in (False, True)]
SPHERE_K = 4


@functools.lru_cache(maxsize=None)
def sphere_reference(level, S, persp, cull=False, K=SPHERE_K):
    """(face_verts, float64 result, float32 restatement) of a sphere case, computed once and shared (read only)."""
    fv, _ = sphere_faces(level)
    F = len(fv)
    r64 = rasterize(fv, [0], [F], S, K, persp, cull, np.float64)
    r32 = rasterize(fv, [0], [F], S, K, persp, cull, np.float32)
    return fv, r64, r32


def stack_scene():
    """Dyadic coordinates (multiples of 1/16; S = 32 puts the centres on odd multiples of 1/32, so every edge function is
    exact in float32): ten parallel triangles over the same pixels at depths 10, 9, .. 1 (the nearest stored last); two
    pairs of identical triangles (equal depth: the tie rule); and a quad split along its diagonal whose corners, outline and
    diagonal pass exactly through pixel centres (the corners are odd multiples of 1/32 themselves): those centres belong to
    neither face.  -> face_verts (F,3,3) float32."""
    faces = []
    tri = np.array([[0.75, -0.75], [-0.75, -0.75], [0.0, 0.75]])
    for k in range(10):
        faces.append(np.concatenate([tri, np.full((3, 1), 10.0 - k)], axis=1))
    small = np.array([[0.5, -0.5], [-0.5, -0.5], [0.0, 0.5]])
    for z in (0.5, 0.5, 5.5, 5.5):                                   # two pairs of identical triangles
        faces.append(np.concatenate([small, np.full((3, 1), z)], axis=1))
    # a split quad far in front of nothing else (x in [-31/32, -15/32], y likewise): corners ON pixel centres
    a, b = -31.0 / 32.0, -15.0 / 32.0
    quad = np.array([[a, a], [b, a], [b, b], [a, b]])
    for idx in ((0, 2, 1), (0, 3, 2)):
        faces.append(np.concatenate([quad[list(idx)], np.full((3, 1), 2.0)], axis=1))
    return np.stack(faces).astype(np.float32)


def heavy_tile_scene(count=3000, seed=3):
    """`count` small faces whose centres lie inside the first 16 x 16 tile of an S = 32 image (NDC x, y in (0, 1)), random
    depths in (1, 9), plus one face covering the whole tile at depth 0.5 stored LAST -> face_verts (count + 1,3,3) float32."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(0.08, 0.92, size=(count, 1, 2))
    # equilateral, randomly turned: a sliver's tol = 16 eps T / |area| is large, and 3000 x 256 pairs of random slivers put
    # more than 1 % of the tile's pixels within tol of some edge line
    ang = rng.uniform(0.0, 2.0 * np.pi, size=(count, 1)) + np.array([[0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0]])
    off = rng.uniform(0.04, 0.07, size=(count, 1, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    z = rng.uniform(1.0, 9.0, size=(count, 1, 1)) + rng.uniform(-0.05, 0.05, size=(count, 3, 1))
    small = np.concatenate([c + off, z], axis=2)
    big = np.array([[[1.5, -0.5, 0.5], [-0.5, -0.5, 0.5], [0.5, 2.5, 0.5]]])
    return np.concatenate([small, big]).astype(np.float32)


def flat_shading(p2f0, bary0, face_verts_world, camera_position, light_direction=None, light_location=None, ambient=0.5,
                 diffuse=0.3, specular=0.2, shininess=64, face_colors=None, background=(1.0, 1.0, 1.0)):
    """float64 numpy restatement of hard_flat_shading's formula for slot 0: p2f0 (N,S,S), bary0 (N,S,S,3) -> (N,S,S,4)."""
    fvw = np.asarray(face_verts_world, dtype=np.float64)
    covered = p2f0 >= 0
    fv = fvw[np.maximum(p2f0, 0)]
    b = np.asarray(bary0, dtype=np.float64)

    def unit(v):
        return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-6)

    n = unit(np.cross(fv[..., 1, :] - fv[..., 0, :], fv[..., 2, :] - fv[..., 0, :]))
    p = (b[..., None] * fv).sum(-2)
    texel = np.ones_like(p) if face_colors is None else (b[..., None] * np.asarray(face_colors, np.float64)[np.maximum(p2f0, 0)]).sum(-2)
    N = p2f0.shape[0]
    per_view = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1, 1, 1, 3), (N, 1, 1, 3))
    if light_location is not None:
        l = unit(per_view(light_location) - p)
    else:
        l = np.broadcast_to(unit(per_view(light_direction if light_direction is not None else (0.0, 1.0, 0.0))), p.shape)
    cos = (n * l).sum(-1, keepdims=True)
    view = unit(per_view(camera_position) - p)
    refl = -l + 2.0 * cos * n
    spec = np.maximum((view * refl).sum(-1, keepdims=True), 0.0) * (cos > 0)
    col = (ambient + diffuse * np.maximum(cos, 0.0)) * texel + specular * spec ** shininess
    rgb = np.where(covered[..., None], col, np.broadcast_to(np.asarray(background, dtype=np.float64), col.shape))
    return np.concatenate([rgb, covered[..., None].astype(np.float64)], axis=-1)
