"""Block-sparse marching tetrahedra restated in numpy: include/isopoints.h section O and DESIGN.md 3.4k on top of
mesh_extract_oracle (section N).  tests/test_mesh_sparse_cpu.py checks it by properties that do not depend on it;
tests/test_mesh_sparse_gpu.py then compares the kernels and ops.sparse_level_set with it.

Brick b holds the grid points 8 b .. 8 b + 7 per axis; cell-block b the cells whose base point lies in brick b.  A block is a
tuple (bx, by, bz); sets of blocks are python sets or sorted lists (by linear index (bx nby + by) nbz + bz).  A slot (p, s)
is live iff one of the cells that contain it -- base p - d, d in {0,1}^3 with d & code(s) == 0 -- exists and lies in a
cell-active block.  Vertices are ordered by (brick of p, local point, slot), faces by (block of the cell, local cell,
tetrahedron, triangle): both are (linear brick index, local index) sorts, so the list of sampled bricks does not enter.
"""
import itertools

import numpy as np

import mesh_extract_oracle as M

B = 8
OFFSETS = tuple(itertools.product((0, 1), repeat=3))              # d = (dx, dy, dz); code = dx + 2 dy + 4 dz


def code(d):
    return d[0] + 2 * d[1] + 4 * d[2]


def brick_dims(shape):
    return tuple((n + B - 1) // B for n in shape)


def brick_lin(b, shape):
    nb = brick_dims(shape)
    return (b[0] * nb[1] + b[1]) * nb[2] + b[2]


def sort_blocks(blocks, shape):
    return sorted({tuple(int(x) for x in b) for b in blocks}, key=lambda b: brick_lin(b, shape))


def all_blocks(shape):
    return sort_blocks(itertools.product(*[range(n) for n in brick_dims(shape)]), shape)


def sampled(blocks, shape):
    """The bricks the cells of `blocks` touch: b + {0,1}^3 where it exists in the grid, sorted."""
    nb = brick_dims(shape)
    out = set()
    for b in blocks:
        for o in OFFSETS:
            q = (b[0] + o[0], b[1] + o[1], b[2] + o[2])
            if all(q[x] < nb[x] for x in range(3)):
                out.add(q)
    return sort_blocks(out, shape)


def marched_cells(shape, blocks):
    """(nx-1, ny-1, nz-1) bool: the cell lies in a block of `blocks`."""
    out = np.zeros(tuple(n - 1 for n in shape), dtype=bool)
    for b in blocks:
        out[tuple(slice(B * b[x], B * b[x] + B) for x in range(3))] = True
    return out


def _cells_of_slot(p, s, shape):
    """The existing cells (as base points) that contain slot s of point p."""
    d_slot = M.SLOTS[s]
    for d in OFFSETS:
        if any(d[x] and d_slot[x] for x in range(3)):
            continue
        c = (p[0] - d[0], p[1] - d[1], p[2] - d[2])
        if all(0 <= c[x] < shape[x] - 1 for x in range(3)):
            yield c


def _active_slots(values, marched, level):
    """[(p, s)] in (p, s) order of the dense linear index: the live slots whose ends differ."""
    ins = M.inside_mask(values, level)
    shape = values.shape
    out = []
    differs = np.zeros(shape, dtype=bool)
    for d in M.SLOTS:
        sl_a = tuple(slice(0, shape[x] - d[x]) for x in range(3))
        sl_b = tuple(slice(d[x], shape[x]) for x in range(3))
        differs[sl_a] |= ins[sl_a] != ins[sl_b]
    for p in np.argwhere(differs):
        p = tuple(int(x) for x in p)
        for s, d in enumerate(M.SLOTS):
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if any(q[x] >= shape[x] for x in range(3)) or ins[p] == ins[q]:
                continue
            if any(marched[c] for c in _cells_of_slot(p, s, shape)):
                out.append((p, s))
    return out


def _local_key(p, shape):
    b = tuple(x // B for x in p)
    return (brick_lin(b, shape), ((p[0] % B) * B + p[1] % B) * B + p[2] % B)


def restrict(values, blocks, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), level=0.0, dtype=np.float32):
    """M.extract restricted to the cells of the cell-active `blocks`, in the sparse order:
    (verts (V,3) dtype, faces (F,3) int64, vert_key (V,) int64 = 7 p + slot, face_cell (F,) int64 = p of the cell)."""
    values = np.asarray(values, dtype=np.float32)
    shape = values.shape
    nx, ny, nz = shape
    ft = np.dtype(dtype).type
    iso = ft(np.float32(level))
    org = [ft(np.float32(o)) for o in origin]
    spc = [ft(np.float32(s)) for s in spacing]
    ins = M.inside_mask(values, level)
    val = values.astype(dtype)
    marched = marched_cells(shape, blocks)

    def lin(p):
        return (p[0] * ny + p[1]) * nz + p[2]

    def pos(idx):
        return [org[d] + ft(idx[d]) * spc[d] for d in range(3)]
    slots = sorted(_active_slots(values, marched, level), key=lambda ps: _local_key(ps[0], shape) + (ps[1],))
    vert_of, verts, keys = {}, [], []
    for p, s in slots:
        d = M.SLOTS[s]
        q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
        va, vb = val[p], val[q]
        if np.isfinite(va) and np.isfinite(vb):
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                t = (iso - va) / (vb - va)
        else:
            t = ft(0.5)
        pa, pb = pos(p), pos(q)
        with np.errstate(over="ignore", invalid="ignore"):
            verts.append([pa[x] + t * (pb[x] - pa[x]) for x in range(3)])
        vert_of[p + (s,)] = len(verts) - 1
        keys.append(7 * lin(p) + s)
    tets = [(M.tet_corners(p), M._perm_sign(p)) for p in M.PERMS]
    cells = sorted((tuple(int(x) for x in c) for c in np.argwhere(marched)), key=lambda c: _local_key(c, shape))
    faces, face_cell = [], []
    for i, j, k in cells:
        corner = [bool(ins[i + d[0], j + d[1], k + d[2]]) for d in OFFSETS]
        if all(corner) or not any(corner):
            continue
        for corners, orient in tets:
            inside = [bool(ins[i + c[0], j + c[1], k + c[2]]) for c in corners]
            for tri in M.tet_triangles(inside, orient):
                f = []
                for u, v in tri:
                    cu, cv = corners[u], corners[v]
                    d = (cv[0] - cu[0], cv[1] - cu[1], cv[2] - cu[2])
                    f.append(vert_of[(i + cu[0], j + cu[1], k + cu[2], M.SLOTS.index(d))])
                faces.append(f)
                face_cell.append(lin((i, j, k)))
    return (np.array(verts, dtype=dtype).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3),
            np.array(keys, dtype=np.int64), np.array(face_cell, dtype=np.int64))


def sort_by_keys(verts, faces, vert_key, face_cell):
    """The sparse mesh in the dense order: vertices by key, faces by cell (stable: tetrahedron and triangle order stay)."""
    order = np.argsort(vert_key, kind="stable")
    new_index = np.empty(len(order), dtype=np.int64)
    new_index[order] = np.arange(len(order))
    forder = np.argsort(face_cell, kind="stable")
    return verts[order], new_index[faces][forder] if len(faces) else faces


def needed(values, blocks, level=0.0):
    """{brick b: need byte}: bit code(o) is set iff a vertex-carrying slot owned by a point of b is also contained in an
    existing cell of block b - o that is not cell-active.  Bricks without a bit are left out."""
    values = np.asarray(values, dtype=np.float32)
    shape = values.shape
    active = {tuple(b) for b in blocks}
    marched = marched_cells(shape, active)
    need = {}
    for p, s in _active_slots(values, marched, level):
        b = tuple(x // B for x in p)
        for c in _cells_of_slot(p, s, shape):
            cb = tuple(x // B for x in c)
            if cb not in active:
                o = (b[0] - cb[0], b[1] - cb[1], b[2] - cb[2])
                need[b] = need.get(b, 0) | (1 << code(o))
    return need


def needed_blocks(need):
    out = set()
    for b, byte in need.items():
        for o in OFFSETS:
            if (byte >> code(o)) & 1:
                out.add((b[0] - o[0], b[1] - o[1], b[2] - o[2]))
    return out


def closure(values, seed_blocks, level=0.0):
    """Apply `needed` until nothing is added: (sorted blocks, rounds), rounds = the number of times `needed` ran."""
    shape = np.asarray(values).shape
    blocks, rounds = {tuple(b) for b in seed_blocks}, 0
    while True:
        rounds += 1
        more = needed_blocks(needed(values, blocks, level)) - blocks
        if not more:
            return sort_blocks(blocks, shape), rounds
        blocks |= more


def blocks_with_cells(shape):
    """The blocks that hold at least one cell: 8 b_d < n_d - 1 on every axis."""
    return [b for b in all_blocks(shape) if all(B * b[x] < shape[x] - 1 for x in range(3))]


def band_seeds(values, spacing, band, level=0.0):
    """The seeding rule on a dense volume: block b (with at least one cell) is a seed iff |f(c) - level| <= band * R_b, c the
    grid point min(8 b + 4, n - 1) per axis and R_b the largest distance from c to a corner of the block's cell region,
    the index range [8 b_d, min(8 b_d + 8, n_d - 1)] per axis."""
    values = np.asarray(values, dtype=np.float32)
    shape = values.shape
    out = []
    for b in blocks_with_cells(shape):
        c = tuple(min(B * b[x] + 4, shape[x] - 1) for x in range(3))
        lo = [B * b[x] for x in range(3)]
        hi = [min(B * b[x] + B, shape[x] - 1) for x in range(3)]
        R = np.sqrt(sum((max(c[x] - lo[x], hi[x] - c[x]) * float(spacing[x])) ** 2 for x in range(3)))
        if abs(float(values[c]) - float(level)) <= band * R:
            out.append(b)
    return out


def sign_change_blocks(values, level=0.0):
    """The blocks that hold a cell whose corners differ in the inside test."""
    ins = M.inside_mask(values, level)
    n = [s - 1 for s in ins.shape]
    total = np.zeros(n, dtype=np.int32)
    for d in OFFSETS:
        total += ins[d[0]:d[0] + n[0], d[1]:d[1] + n[1], d[2]:d[2] + n[2]]
    return sort_blocks({tuple(int(x) // B for x in c) for c in np.argwhere((total > 0) & (total < 8))}, ins.shape)


def to_bricks(values, bricks):
    """The dense volume gathered into (S, 8, 8, 8) float32 for the listed bricks; entries outside the grid are NaN."""
    values = np.asarray(values, dtype=np.float32)
    out = np.full((len(bricks), B, B, B), np.nan, dtype=np.float32)
    for s, b in enumerate(bricks):
        part = values[tuple(slice(B * b[x], B * b[x] + B) for x in range(3))]
        out[(s,) + tuple(slice(0, n) for n in part.shape)] = part
    return out


def boundary_edges(faces):
    """The edges that are not in exactly two faces, once in each direction."""
    return [e for e, c in M.edge_census(faces).items() if c != [1, 1]]
