"""The numpy restatement of block-sparse marching tetrahedra (tests/mesh_sparse_oracle.py; include/isopoints.h section O)
checked without a GPU, by properties that do not depend on it: against the dense restatement where all blocks are active,
and by the open edges of the restricted mesh where they are not.  tests/test_mesh_sparse_gpu.py compares the kernels with
it element for element."""
import functools

import numpy as np
import pytest

import mesh_extract_oracle as M
import mesh_sparse_oracle as S


# two_spheres on 36^3 over a box of side 2.2 has one block, (2, 2, 2), that holds the facing tips of both spheres (they are
# 0.2 apart, a block is 0.5 wide): marching that block's cells meets both surfaces, and the closure rightly follows both.
# On this grid the brick boundary at index 24 is the plane x = 0.15, between the tips at x = 0.05 and x = 0.25, so no
# block holds cells of both spheres.
SPLIT_GRID = ((40, 40, 40), (0.15 - 24 * 0.06, -1.17, -1.17), (0.06, 0.06, 0.06))


def _boxed(sdf, n, side=2.0):
    shape, org, spc = M.box_grid(n, side)
    return M.volume(sdf, shape, org, spc), org, spc


@functools.lru_cache(maxsize=None)
def volume(name):
    if name == "sphere33":
        out = _boxed(lambda p: M.sphere_sdf(p, 0.6), 33)
    elif name == "two_spheres":
        out = _boxed(M.two_spheres_sdf, 36, 2.2)
    elif name == "two_spheres_apart":
        out = M.volume(M.two_spheres_sdf, *SPLIT_GRID), SPLIT_GRID[1], SPLIT_GRID[2]
    elif name == "cut_sphere":
        out = _boxed(lambda p: M.sphere_sdf(p, 1.2), 21)
    else:
        shape, org, spc = (20, 27, 35), (-0.9, -1.0, -1.1), (0.1, 0.08, 0.065)
        out = M.volume(lambda p: M.sphere_sdf(p, 0.7), shape, org, spc), org, spc
    out[0].setflags(write=False)
    return out


@pytest.mark.parametrize("name", ["sphere33", "two_spheres", "cut_sphere", "ragged"])
def test_all_blocks_give_the_dense_mesh(name):
    vol, org, spc = volume(name)
    want_v, want_f = M.extract(vol, org, spc)
    v, f, vk, fc = S.restrict(vol, S.all_blocks(vol.shape), org, spc)
    assert len(want_f) > 0 and v.shape == want_v.shape and f.shape == want_f.shape
    assert len(np.unique(vk)) == len(vk) and sorted(np.unique(f)) == list(range(len(v)))
    got_v, got_f = S.sort_by_keys(v, f, vk, fc)
    assert np.array_equal(got_v.view(np.int32), want_v.view(np.int32)) and np.array_equal(got_f, want_f)
    assert not S.needed(vol, S.all_blocks(vol.shape))
    # the sparse order is not the dense one: bricks come before rows of the grid
    assert not np.array_equal(vk, np.sort(vk))
    nb = S.brick_dims(vol.shape)
    brick = lambda p: ((p // (vol.shape[1] * vol.shape[2]) // 8) * nb[1] + (p // vol.shape[2] % vol.shape[1]) // 8) * nb[2] + p % vol.shape[2] // 8
    assert (np.diff(brick(vk // 7)) >= 0).all() and (np.diff(brick(fc)) >= 0).all()


def _on_a_grid_face(verts, a, b, org, spc, shape):
    """both ends of the edge on one face of the grid"""
    lo = np.array(org, dtype=np.float64)
    hi = lo + (np.array(shape) - 1) * np.array(spc, dtype=np.float64)
    on_a = (np.abs(verts[a] - lo) < 1e-6) | (np.abs(verts[a] - hi) < 1e-6)
    on_b = (np.abs(verts[b] - lo) < 1e-6) | (np.abs(verts[b] - hi) < 1e-6)
    return bool((on_a & on_b).any())


@pytest.mark.parametrize("name", ["sphere33", "cut_sphere", "ragged"])
def test_need_is_empty_iff_the_mesh_is_open_on_the_grid_faces_only(name):
    """Subsets of the blocks, from a single one up to the closure: wherever `needed` reports nothing every open edge of the
    restricted mesh lies on a face of the grid, and wherever it reports something there is an open edge inside."""
    vol, org, spc = volume(name)
    change = S.sign_change_blocks(vol)
    rng = np.random.default_rng(3)
    picks = [[change[0]], [change[len(change) // 2]], [b for b in change if rng.random() < 0.5],
             [b for b in S.all_blocks(vol.shape) if sum(b) % 2 == 0], S.closure(vol, [change[0]])[0], change]
    seen = set()
    for blocks in picks:
        v, f, _vk, _fc = S.restrict(vol, blocks, org, spc)
        inner = [e for e in S.boundary_edges(f) if not _on_a_grid_face(v, e[0], e[1], org, spc, vol.shape)]
        need = S.needed(vol, blocks)
        assert bool(need) == bool(inner), (name, len(blocks), len(need), len(inner))
        seen.add(bool(need))
        assert not (S.needed_blocks(need) & {tuple(b) for b in blocks})          # only blocks that are not active yet
        for b in S.needed_blocks(need):
            assert all(0 <= b[x] < S.brick_dims(vol.shape)[x] for x in range(3))
    assert seen == {True, False}


def test_band_one_covers_every_sign_change_on_the_sphere():
    """The condition the GPU equality tests rest on: for an exact SDF band = 1 is conservative."""
    vol, org, spc = volume("sphere33")
    seeds = set(S.band_seeds(vol, spc, band=1.0))
    change = set(S.sign_change_blocks(vol))
    assert change and change <= seeds and len(seeds) < len(S.all_blocks(vol.shape))
    assert set(S.band_seeds(vol, spc, band=0.0)) == set()
    assert not S.needed(vol, seeds)


def test_closure_from_one_block_takes_the_first_sphere_only():
    vol, org, spc = volume("two_spheres_apart")
    centre = np.array([-0.4, 0.0, 0.0])
    pts = M.grid_points(vol.shape, org, spc).astype(np.float64)
    near_first = M.sphere_sdf(pts, 0.45, centre) < M.sphere_sdf(pts, 0.3, (0.55, 0.1, 0.0))
    change = S.sign_change_blocks(vol)
    first = [b for b in change if near_first[min(8 * b[0] + 4, vol.shape[0] - 1), min(8 * b[1] + 4, vol.shape[1] - 1),
                                             min(8 * b[2] + 4, vol.shape[2] - 1)]]
    assert 0 < len(first) < len(change)
    blocks, rounds = S.closure(vol, [first[0]])
    assert rounds > 2 and not S.needed(vol, blocks)
    v, f, vk, fc = S.restrict(vol, blocks, org, spc)
    assert M.is_closed_and_oriented(f) and M.euler_characteristic(f) == 2
    r = np.linalg.norm(v.astype(np.float64) - centre, axis=1)
    assert np.abs(r - 0.45).max() < 0.01
    # exactly the first sphere's blocks: every block with one of its sign changes, and no block of the second sphere
    with_faces = {tuple(int(x) // 8 for x in np.unravel_index(c, vol.shape)) for c in fc}
    assert with_faces <= set(blocks) and not (set(blocks) & (set(change) - with_faces))
    dense_v, dense_f = M.extract(vol, org, spc)
    lab = M.components(dense_f)
    sizes = [int((lab == c).sum()) for c in (0, 1)]
    assert len(f) in sizes and len(f) < len(dense_f)


def test_a_block_that_holds_both_spheres_joins_them():
    """The other side of the rule: a cell-active block marches all of its cells, so on the 36^3 grid, where block (2, 2, 2)
    holds the tips of both spheres, the closure from the first sphere ends with both."""
    vol, org, spc = volume("two_spheres")
    blocks, _rounds = S.closure(vol, [S.sign_change_blocks(vol)[0]])
    assert (2, 2, 2) in blocks and set(blocks) == set(S.sign_change_blocks(vol))
    v, f, vk, fc = S.restrict(vol, blocks, org, spc)
    assert M.is_closed_and_oriented(f) and M.euler_characteristic(f) == 4
