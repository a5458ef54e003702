"""Marching tetrahedra on the Kuhn split, restated in numpy: include/isopoints.h section N and DESIGN.md 3.4j, as plain
loops over the grid.  tests/test_mesh_extract_cpu.py checks it by properties that do not depend on it (closed, oriented,
Euler characteristic, on the surface); tests/test_mesh_extract_gpu.py then compares the kernels with it element for element.

The rule.  Grid point (i, j, k) lies at origin + (i, j, k) * spacing and has linear index (i * ny + j) * nz + k.  A point is
inside iff its value is finite and < iso.  Every point owns 7 slots, the mesh edges that START there, in the order
+x, +y, +z, +xy, +xz, +yz, +xyz; a slot exists if its far end is in the grid and is active if exactly one end is inside.
An active slot carries the vertex pa + t * (pb - pa), t = (iso - va) / (vb - va), a the owning end (t = 0.5 if an end is
not finite).  Vertices are numbered in (point, slot) order.  A cell is cut into the six tetrahedra 000 -> +e_a ->
+e_a+e_b -> 111, (a, b, c) the permutations of the axes in lexicographic order; a tetrahedron with one or three corners
inside gives one triangle, with two a quad cut along the diagonal from (lower inside, lower outside) to (higher inside,
higher outside); every triangle is wound so that its right-hand normal points to the outside corners.  Faces are
ordered by cell, tetrahedron, triangle.
"""
import itertools

import numpy as np

SLOTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))                    # lexicographic


def _perm_sign(p):
    p, s = list(p), 1
    for i in range(len(p)):
        for j in range(i + 1, len(p)):
            if p[i] > p[j]:
                s = -s
    return s


def tet_corners(perm):
    """The four corners of the tetrahedron of one axis permutation, as offsets in the cell."""
    a, b, _c = perm
    p1 = [0, 0, 0]
    p1[a] = 1
    p2 = list(p1)
    p2[b] = 1
    return ((0, 0, 0), tuple(p1), tuple(p2), (1, 1, 1))


def tet_triangles(inside, orientation):
    """Triangles of one tetrahedron.  inside: 4 booleans; orientation: sign of det[P1-P0, P2-P0, P3-P0].  Each triangle
    is three tetrahedron edges (u, v), u < v.  With A the lone corner and B < C < D the others, the normal of (AB, AC, AD)
    points away from A iff det[B-A, C-A, D-A] > 0; with A < B inside and C < D outside the normal of the quad (AC, AD, BD,
    BC) points to C and D under the same condition; that determinant is orientation * sign of the permutation (A, B, C, D)."""
    ins = [q for q in range(4) if inside[q]]
    out = [q for q in range(4) if not inside[q]]

    def e(u, v):
        return (min(u, v), max(u, v))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(ins) == 3:
        lone = ins[0] if len(ins) == 1 else out[0]
        rest = out if len(ins) == 1 else ins
        away = orientation * _perm_sign([lone] + rest) > 0          # (AB, AC, AD) points away from the lone corner
        tri = [e(lone, rest[0]), e(lone, rest[1]), e(lone, rest[2])]
        if away != (len(ins) == 1):                                 # lone inside: away from it; lone outside: towards it
            tri = [tri[0], tri[2], tri[1]]
        return [tri]
    (A, B), (C, D) = ins, out
    quad = [e(A, C), e(A, D), e(B, D), e(B, C)]
    tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    if orientation * _perm_sign([A, B, C, D]) < 0:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return tris


def inside_mask(values, level):
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v < np.float32(level))


def extract(values, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), level=0.0, dtype=np.float32):
    """(verts (V,3) dtype, faces (F,3) int64).  dtype float32 is the kernels' arithmetic, one rounding per operation;
    float64 is the same rule on the same float32 values and the float32 level."""
    values = np.asarray(values, dtype=np.float32)
    nx, ny, nz = values.shape
    ft = np.dtype(dtype).type
    iso = ft(np.float32(level))
    org = [ft(np.float32(o)) for o in origin]
    spc = [ft(np.float32(s)) for s in spacing]
    ins = inside_mask(values, level)
    val = values.astype(dtype)
    dims = (nx, ny, nz)

    def pos(idx):
        return [org[d] + ft(idx[d]) * spc[d] for d in range(3)]

    # vertices: (point, slot) order
    vert_of = {}
    verts = []
    active_points = np.zeros(dims, dtype=bool)                      # any neighbour of the cell at this point differs
    for d in SLOTS:
        sl_a = tuple(slice(0, dims[x] - d[x]) for x in range(3))
        sl_b = tuple(slice(d[x], dims[x]) for x in range(3))
        active_points[sl_a] |= ins[sl_a] != ins[sl_b]
    for i, j, k in np.argwhere(active_points):                      # argwhere is in linear-index order
        for s, d in enumerate(SLOTS):
            b = (i + d[0], j + d[1], k + d[2])
            if b[0] >= nx or b[1] >= ny or b[2] >= nz or ins[i, j, k] == ins[b]:
                continue
            va, vb = val[i, j, k], val[b]
            if np.isfinite(va) and np.isfinite(vb):
                with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                    t = (iso - va) / (vb - va)
            else:
                t = ft(0.5)
            pa, pb = pos((i, j, k)), pos(b)
            with np.errstate(over="ignore", invalid="ignore"):
                verts.append([pa[x] + t * (pb[x] - pa[x]) for x in range(3)])
            vert_of[(i, j, k, s)] = len(verts) - 1

    # faces: cell, tetrahedron, triangle
    tets = [(tet_corners(p), _perm_sign(p)) for p in PERMS]
    faces = []
    cell_active = active_points[:-1, :-1, :-1]
    for i, j, k in np.argwhere(cell_active):
        for corners, orient in tets:
            inside = [bool(ins[i + c[0], j + c[1], k + c[2]]) for c in corners]
            for tri in tet_triangles(inside, orient):
                f = []
                for u, v in tri:
                    cu, cv = corners[u], corners[v]
                    d = (cv[0] - cu[0], cv[1] - cu[1], cv[2] - cu[2])
                    f.append(vert_of[(i + cu[0], j + cu[1], k + cu[2], SLOTS.index(d))])
                faces.append(f)
    return (np.array(verts, dtype=dtype).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3))


# ----------------------------------------------------------------------------- properties, from the arrays alone
def edge_census(faces):
    """{(lo, hi): [number of faces that run lo -> hi, number that run hi -> lo]}"""
    census = {}
    for f in np.asarray(faces):
        for u, v in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            key = (min(u, v), max(u, v))
            census.setdefault(key, [0, 0])[0 if u < v else 1] += 1
    return census


def is_closed_and_oriented(faces):
    return all(c == [1, 1] for c in edge_census(faces).values())


def euler_characteristic(faces):
    faces = np.asarray(faces)
    return len(np.unique(faces)) - len(edge_census(faces)) + len(faces)


def face_normals_areas(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    return n, 0.5 * np.linalg.norm(n, axis=1)


def components(faces):
    """Label per face by connectivity over shared vertex indices (union-find), labels 0.. in order of first face."""
    faces = np.asarray(faces)
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for f in faces:
        r = find(f[0])
        parent[find(f[1])] = r
        parent[find(f[2])] = r
    roots, labels = {}, []
    for f in faces:
        labels.append(roots.setdefault(find(f[0]), len(roots)))
    return np.array(labels, dtype=np.int64)


# ----------------------------------------------------------------------------- test volumes
def grid_axes(shape, origin, spacing):
    return [np.float32(origin[d]) + np.arange(shape[d], dtype=np.float32) * np.float32(spacing[d]) for d in range(3)]


def grid_points(shape, origin, spacing):
    x, y, z = grid_axes(shape, origin, spacing)
    return np.stack(np.meshgrid(x, y, z, indexing="ij"), axis=-1)     # (nx, ny, nz, 3) float32


def box_grid(n, side=2.0):
    """n^3 points over [-side/2, side/2]^3: (shape, origin, spacing)"""
    return (n, n, n), (-side / 2,) * 3, (side / (n - 1),) * 3


def sphere_sdf(p, radius, center=(0.0, 0.0, 0.0)):
    p = np.asarray(p, dtype=np.float64)
    return np.linalg.norm(p - np.asarray(center, dtype=np.float64), axis=-1) - radius


def torus_sdf(p, R, r):
    p = np.asarray(p, dtype=np.float64)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return np.sqrt(q ** 2 + p[..., 2] ** 2) - r


def torus_grad(p, R, r):
    p = np.asarray(p, dtype=np.float64)
    rho = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)
    q = rho - R
    d = np.sqrt(q ** 2 + p[..., 2] ** 2)
    return np.stack([q * p[..., 0] / rho, q * p[..., 1] / rho, p[..., 2]], axis=-1) / d[..., None]


def two_spheres_sdf(p):
    """radius 0.45 about (-0.4, 0, 0) and radius 0.3 about (0.55, 0.1, 0): disjoint, the first the larger"""
    return np.minimum(sphere_sdf(p, 0.45, (-0.4, 0.0, 0.0)), sphere_sdf(p, 0.3, (0.55, 0.1, 0.0)))


def volume(sdf, shape, origin, spacing):
    return sdf(grid_points(shape, origin, spacing)).astype(np.float32)
