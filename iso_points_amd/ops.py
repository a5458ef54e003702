"""Points and normals sampled on meshes: pytorch3d.ops.sample_points_from_meshes as the reference calls it
(evaluation.py:113 and :164 -- the clouds that chamfer_p / chamfer_n / pf_dist grade; scripts/create_mvr_data_from_mesh.py:171;
tests/test_projection.py:347), and pytorch3d.ops.mesh_face_areas_normals.

One host-side seed per call, everything else counter-based inside the kernel (Philox4x32-10 on (seed, mesh, sample)): a
sample does not depend on num_samples, on the other meshes or on a launch shape.  The backward pass is the gather over
counting-sorted lists of the loss module: no float atomics, values and gradients are the same bits from run to run
(include/isopoints.h section I).

sample_points_from_meshes_even is the even sampling the reference takes from trimesh.sample.sample_surface_even
(config.py:227, DSS/training/trainer.py:255) and pcu.sample_mesh_poisson_disk (DSS/utils/dataset.py:123): the same draw, three
times as long, followed by the Poisson-disk elimination of include/isopoints.h section L.

marching_tetrahedra, sdf_grid, mesh_components / largest_component and get_surface_high_res_mesh are the way back: the
model's level set as a mesh, where the reference runs skimage's marching cubes and trimesh on the host
(DSS/utils/__init__.py:569-700; include/isopoints.h section N).
"""
import contextlib
import math

import numpy as np
import torch

from . import _lib
from .loss import _on_gpu, _packed_mesh
from .mesh_raster import (Fragments, MeshRasterizer, RasterizationSettings, hard_flat_shading,  # noqa: F401
                          rasterize_meshes, render_views)

_ROW_LIMIT = 2 ** 31


class _MeshSample(torch.autograd.Function):
    """tris (T,3,3) -> points (N,S,3), normals (N,S,3) or None, face_idx (N,S) int32 and bary (N,S,3) (constants; None
    unless asked for or needed by the backward pass)."""

    @staticmethod
    def forward(ctx, tris, first, length, S, seed, want_normals, want_faces):
        N, T, dev = first.shape[0], tris.shape[0], tris.device
        keep = want_faces or ctx.needs_input_grad[0]
        points = torch.empty((N, S, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((N, S, 3), dtype=torch.float32, device=dev) if want_normals else None
        face = torch.empty((N, S), dtype=torch.int32, device=dev) if keep else None
        bary = torch.empty((N, S, 3), dtype=torch.float32, device=dev) if keep else None
        ws_bytes = _lib.load().iso_mesh_sample_workspace_bytes(N, T)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        p = _lib.ptr
        _lib.call("iso_mesh_sample", p(tris), p(first), p(length), N, T, S, seed, p(points), p(normals), p(face), p(bary),
                  p(ws), ws_bytes, _lib.stream())
        ctx.save_for_backward(tris, face, bary)
        ctx.want_normals = want_normals
        if keep:
            ctx.mark_non_differentiable(face, bary)
        return points, normals, face, bary

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_points, g_normals, _g_face, _g_bary):
        tris, face, bary = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        grad = torch.empty_like(tris)
        T, rows = tris.shape[0], face.numel()
        if T == 0:
            return (grad,) + (None,) * 6
        g_points = g_points.detach().float().contiguous()
        g_normals = g_normals.detach().float().contiguous() if ctx.want_normals and g_normals is not None else None
        ws_bytes = _lib.load().iso_mesh_sample_backward_workspace_bytes(T, rows)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=tris.device)
        p = _lib.ptr
        _lib.call("iso_mesh_sample_backward", p(tris), p(face), p(bary), p(g_points), p(g_normals), p(grad), T, rows, p(ws),
                  ws_bytes, _lib.stream())
        return (grad,) + (None,) * 6


def sample_points_from_meshes(meshes, num_samples=10000, return_normals=False, return_textures=False, *, generator=None,
                              return_faces=False):
    """pytorch3d.ops.sample_points_from_meshes: `num_samples` points on every mesh of the batch, uniform over its surface
    (a face with probability area / total area, a point uniform inside the face).  Returns points (N,S,3) float32; with
    return_normals also normals (N,S,3), the unit normal of each sample's face; with return_faces also face_idx (N,S) int64
    into the packed faces and bary (N,S,3) float32, the weights of the face's three vertices.

    `meshes` is an object with verts_packed / faces_packed / mesh_to_faces_packed_first_idx / num_faces_per_mesh or a
    (verts (N,V,3), faces (N,F,3) integer[, num_faces]) tuple.  A mesh without faces or without area gets zero points and
    normals, face_idx = -1 and bary = 0: nothing is read back from the device to find out.  return_textures is not
    supported.

    The call draws one int64 seed on the host from `generator` (a CPU generator; torch's default one without, so
    torch.manual_seed governs the call); sample s of mesh n is a function of (seed, n, s) and that mesh alone, so the first
    k samples of a larger request are the smaller request.  Differentiable w.r.t. the vertices through points and normals,
    with the faces and weights held constant; values and gradients are the same bits from run to run.  Limits, refused
    beyond: fewer than 2^31 packed faces and fewer than 2^31 samples in all."""
    fn = "sample_points_from_meshes"
    if return_textures:
        raise NotImplementedError("%s: textures are not supported" % fn)
    S = int(num_samples)
    if S < 0:
        raise ValueError("%s: num_samples must not be negative" % fn)
    tris, first = _packed_mesh(meshes, fn)
    if not torch.is_tensor(first) or first.dim() != 1 or first.is_floating_point():
        raise ValueError("%s: mesh_to_faces_packed_first_idx must be an integer tensor of shape (N,)" % fn)
    N, T = first.shape[0], tris.shape[0]
    if T >= _ROW_LIMIT:
        raise ValueError("%s: %d packed faces; the limit is 2^31 - 1" % (fn, T))
    if N * S >= _ROW_LIMIT:
        raise ValueError("%s: %d meshes x %d samples; the limit is 2^31 - 1 samples in all" % (fn, N, S))
    _on_gpu(tris)
    dev = tris.device
    seed = int(torch.empty((), dtype=torch.int64).random_(generator=generator))
    if N == 0 or S == 0:
        points = tris.new_zeros((N, S, 3), dtype=torch.float32)
        out = (points, torch.zeros_like(points)) if return_normals else (points,)
        if return_faces:
            out = out + (torch.zeros((N, S), dtype=torch.int64, device=dev), torch.zeros_like(points))
        return out if len(out) > 1 else out[0]
    first = first.to(device=dev, dtype=torch.int64).contiguous()
    end = torch.full((1,), T, dtype=torch.int64, device=dev)
    length = (torch.cat([first[1:], end]) - first).contiguous()
    points, normals, face, bary = _MeshSample.apply(tris.float().contiguous(), first, length, S, seed, bool(return_normals),
                                                    bool(return_faces))
    out = (points, normals) if return_normals else (points,)
    if return_faces:
        out = out + (face.long(), bary)
    return out if len(out) > 1 else out[0]


def sample_points_from_meshes_even(meshes, num_samples=10000, radius=None, return_normals=False, *, generator=None,
                                   return_faces=False, oversample=3):
    """An even sampling of every mesh of the batch: up to `num_samples` points no two of which are within `radius` of each
    other, where the reference calls trimesh.sample.sample_surface_even (config.py:227, DSS/training/trainer.py:255) or
    pcu.sample_mesh_poisson_disk (DSS/utils/dataset.py:123).  Not bit for bit theirs: the rule is exact and its own.

    The call draws oversample * num_samples samples per mesh exactly as sample_points_from_meshes(meshes, oversample *
    num_samples, generator=generator) would (one seed taken from the generator, the same bits), marks the samples without a
    face invalid and eliminates in draw order (point_processing.remove_close: a sample is kept iff no kept earlier sample is
    within the radius, d2 <= r * r in float32).  radius: a positive finite float, an (N,) tensor, or None for
    sqrt(area / (3 num_samples)) per mesh from the float64 sum of the float32 face areas, computed on the device.

    Returns (points (N,S,3), num_points (N,) int64[, normals (N,S,3)][, face_idx (N,S) int64, bary (N,S,3)]): the first
    num_points[n] rows are the first kept draws of mesh n in draw order; rows beyond are zero (face_idx -1).  A mesh may
    yield fewer than S points, a mesh without faces or without area yields none.  As both steps are prefix-stable the
    result is a function of (seed, mesh, radius): its first rows do not depend on how many samples were drawn beyond those
    that decided them, so a larger `oversample` changes nothing in the rows a smaller one filled.

    Differentiable w.r.t. the vertices: the outputs are a torch.gather of the sampler's outputs by constant indices, each
    draw taken at most once (the padding rows add exact zeros), so values and gradients are the same bits from run to run.
    Host reads: the 4 bytes per batch of elimination rounds that remove_close reads, normally once.  Limit, refused
    beyond: N * oversample * num_samples < 2^31."""
    from .point_processing import _eliminate
    fn = "sample_points_from_meshes_even"
    S, over = int(num_samples), int(oversample)
    if S < 0:
        raise ValueError("%s: num_samples must not be negative" % fn)
    if over < 1:
        raise ValueError("%s: oversample must be at least 1" % fn)
    tris, first = _packed_mesh(meshes, fn)
    if not torch.is_tensor(first) or first.dim() != 1 or first.is_floating_point():
        raise ValueError("%s: mesh_to_faces_packed_first_idx must be an integer tensor of shape (N,)" % fn)
    N, T, D = first.shape[0], tris.shape[0], over * S
    if torch.is_tensor(radius):
        if radius.dim() != 1 or radius.shape[0] != N:
            raise ValueError("%s: a radius tensor must be of shape (N,)" % fn)
    elif radius is not None:
        radius = float(radius)
        if not (radius > 0.0 and math.isfinite(radius)):
            raise ValueError("%s: radius must be positive and finite, got %r" % (fn, radius))
    if T >= _ROW_LIMIT:
        raise ValueError("%s: %d packed faces; the limit is 2^31 - 1" % (fn, T))
    if N * D >= _ROW_LIMIT:
        raise ValueError("%s: %d meshes x %d x %d draws; the limit is 2^31 - 1 draws in all" % (fn, N, over, S))
    _on_gpu(tris, radius if torch.is_tensor(radius) else None)
    dev = tris.device
    seed = int(torch.empty((), dtype=torch.int64).random_(generator=generator))
    if N == 0 or S == 0:
        points = tris.new_zeros((N, S, 3), dtype=torch.float32)
        out = (points, torch.zeros((N,), dtype=torch.int64, device=dev))
        if return_normals:
            out = out + (torch.zeros_like(points),)
        if return_faces:
            out = out + (torch.full((N, S), -1, dtype=torch.int64, device=dev), torch.zeros_like(points))
        return out
    first = first.to(device=dev, dtype=torch.int64).contiguous()
    end = torch.full((1,), T, dtype=torch.int64, device=dev)
    length = (torch.cat([first[1:], end]) - first).contiguous()
    tris32 = tris.float().contiguous()
    points, normals, face, bary = _MeshSample.apply(tris32, first, length, D, seed, bool(return_normals), True)
    p = _lib.ptr
    if radius is None:
        areas = torch.empty((T,), dtype=torch.float32, device=dev)
        rad = torch.empty((N,), dtype=torch.float32, device=dev)
        _lib.call("iso_mesh_face_areas", p(tris32.detach()), T, p(areas), None, _lib.stream())
        _lib.call("iso_disk_area_radius", p(areas), p(first), p(length), N, T, S, p(rad), _lib.stream())
    elif torch.is_tensor(radius):
        rad = radius.detach().to(device=dev, dtype=torch.float32).contiguous()
    else:
        rad = torch.full((N,), radius, dtype=torch.float32, device=dev)
    lens = torch.full((N,), D, dtype=torch.int64, device=dev)
    _, sel, kept, _ = _eliminate(points.detach().contiguous(), lens, rad, (face >= 0).to(torch.uint8).contiguous(), S)
    live = sel >= 0
    idx = sel.clamp(min=0).long()

    def take(x, pad):
        if x.dim() == 2:
            return torch.where(live, torch.gather(x, 1, idx), x.new_full((), pad))
        return torch.where(live[..., None], torch.gather(x, 1, idx[..., None].expand(N, S, x.shape[-1])), x.new_full((), pad))
    out = (take(points, 0.0), kept)
    if return_normals:
        out = out + (take(normals, 0.0),)
    if return_faces:
        out = out + (take(face, -1).long(), take(bary, 0.0))
    return out


def mesh_face_areas_normals(verts, faces):
    """pytorch3d.ops.mesh_face_areas_normals on packed inputs verts (V,3), faces (F,3) integer: (areas (F,), unit normals
    (F,3)), float32: area = |(v1 - v0) x (v2 - v0)| / 2, normal = the cross product over max(its length, 2.2e-16).  No
    gradient."""
    fn = "mesh_face_areas_normals"
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[-1] != 3:
        raise ValueError("%s: verts must be (V, 3)" % fn)
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[-1] != 3 or faces.is_floating_point():
        raise ValueError("%s: faces must be an integer tensor (F, 3)" % fn)
    if faces.shape[0] >= _ROW_LIMIT:
        raise ValueError("%s: %d faces; the limit is 2^31 - 1" % (fn, faces.shape[0]))
    _on_gpu(verts, faces)
    tris = verts.detach()[faces.long()].float().contiguous()
    F = tris.shape[0]
    areas = torch.empty((F,), dtype=torch.float32, device=tris.device)
    normals = torch.empty((F, 3), dtype=torch.float32, device=tris.device)
    _lib.call("iso_mesh_face_areas", _lib.ptr(tris), F, _lib.ptr(areas), _lib.ptr(normals), _lib.stream())
    return areas, normals


# ----------------------------------------------------------------------------- the level set as a mesh
_GRID_MAX = 1024


def marching_tetrahedra(values, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), level=0.0):
    """The level set {values = level} of a volume sampled on a regular grid as an indexed triangle mesh: (verts (V,3)
    float32, faces (F,3) int64), where the reference calls skimage.measure.marching_cubes_lewiner
    (DSS/utils/__init__.py:582, :635).  Marching tetrahedra on the Kuhn split, not Lewiner's cubes: every vertex lies on
    a grid edge or a cell's face / body diagonal at the zero of the linear interpolant, about twice as many faces, closed
    and consistently oriented wherever the surface does not leave the grid (include/isopoints.h section N has the rule).

    values (nx,ny,nz), each n in [2, 1024]; grid point (i,j,k) lies at origin + (i,j,k) * spacing (three floats each,
    spacing > 0).  A point is inside iff its value is finite and < level; normals point to larger values.  Vertices and
    faces come in a fixed order (by owning grid point and slot; by cell, tetrahedron, triangle) and the same input gives
    the same bits on every run.  A volume without a sign change gives (0,3) tensors.  Faces without area (a value exactly
    on the level) are kept.  Host reads: the two totals, to size the outputs (the library reads the same 16 bytes once
    more to check the outputs' sizes).  No gradient."""
    fn = "marching_tetrahedra"
    if not torch.is_tensor(values) or values.dim() != 3:
        raise ValueError("%s: values must be a (nx, ny, nz) tensor" % fn)
    nx, ny, nz = values.shape
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > _GRID_MAX:
        raise ValueError("%s: every side must be in [2, %d], got %d x %d x %d" % (fn, _GRID_MAX, nx, ny, nz))
    org, spc, level = [float(o) for o in origin], [float(s) for s in spacing], float(level)
    if len(org) != 3 or len(spc) != 3 or not all(math.isfinite(o) for o in org) or \
            not all(s > 0.0 and math.isfinite(s) for s in spc) or not math.isfinite(level):
        raise ValueError("%s: origin and spacing are three finite floats each, spacing > 0, and level is finite" % fn)
    _on_gpu(values)
    vol = values.detach().float().contiguous()
    dev = vol.device
    ws_bytes = _lib.load().iso_meshextract_workspace_bytes(nx, ny, nz)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    p = _lib.ptr
    _lib.call("iso_meshextract_count", p(vol), nx, ny, nz, level, p(totals), p(ws), ws_bytes, _lib.stream())
    V, F = totals.tolist()
    if V >= _ROW_LIMIT or F >= _ROW_LIMIT:
        raise ValueError("%s: %d vertices and %d faces; the limit is 2^31 - 1 of each" % (fn, V, F))
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    _lib.call("iso_meshextract_emit", p(vol), nx, ny, nz, org[0], org[1], org[2], spc[0], spc[1], spc[2], level, p(totals),
              p(verts) if V else None, V, p(faces) if F else None, F, p(ws), ws_bytes, _lib.stream())
    return verts, faces.long()


# ----------------------------------------------------------------------------- ... block-sparse (section O)
_SPARSE_MAX = 4096
_BRICK = 8
_OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1))    # index = x + 2 y + 4 z


def _grid_args(fn, grid_size, origin, spacing, level):
    size = [int(n) for n in grid_size]
    if len(size) != 3 or min(size) < 2 or max(size) > _SPARSE_MAX:
        raise ValueError("%s: grid_size is three sides in [2, %d], got %r" % (fn, _SPARSE_MAX, tuple(grid_size)))
    org, spc, level = [float(o) for o in origin], [float(s) for s in spacing], float(level)
    if len(org) != 3 or len(spc) != 3 or not all(math.isfinite(o) for o in org) or \
            not all(s > 0.0 and math.isfinite(s) for s in spc) or not math.isfinite(level):
        raise ValueError("%s: origin and spacing are three finite floats each, spacing > 0, and level is finite" % fn)
    return size, org, spc, level


def _brick_dims(size):
    return [(n + _BRICK - 1) // _BRICK for n in size]


def _brick_lin(coords, nb):
    c = coords.long()
    return (c[:, 0] * nb[1] + c[:, 1]) * nb[2] + c[:, 2]


def _brick_unlin(lin, nb):
    return torch.stack([lin // (nb[1] * nb[2]), (lin // nb[2]) % nb[1], lin % nb[2]], dim=1)


def _upper_neighbours(lin, nb):
    """The bricks b + {0,1}^3 of the blocks `lin` that exist in the grid: sorted unique linear indices."""
    b = _brick_unlin(lin, nb)
    off = torch.tensor(_OFFSETS, dtype=torch.int64, device=lin.device)
    q = (b[:, None, :] + off[None]).reshape(-1, 3)
    lim = torch.tensor(nb, dtype=torch.int64, device=lin.device)
    q = q[(q < lim).all(dim=1)]
    return torch.unique((q[:, 0] * nb[1] + q[:, 1]) * nb[2] + q[:, 2])


class _SparseCount:
    """One count pass on a sorted brick list: the workspace, need (S,) uint8 and totals (4,) int64 = vertices, faces, set
    need bits, bricks outside the grid, all on the device; emit() then writes the mesh."""

    def __init__(self, values, coords, cell_active, size, level):
        S, dev = coords.shape[0], values.device
        self.args = (values, coords, cell_active, S, size, level)
        self.ws_bytes = _lib.load().iso_meshextract_sparse_workspace_bytes(size[0], size[1], size[2], S)
        if self.ws_bytes <= 0:
            raise ValueError("marching_tetrahedra_bricks: %d bricks on a %d x %d x %d grid are outside the limits "
                             "(sides in [2, %d], fewer than 2^31 / 512 bricks)" % (S, size[0], size[1], size[2], _SPARSE_MAX))
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=dev)
        self.need = torch.empty((S,), dtype=torch.uint8, device=dev)
        self.totals = torch.empty((4,), dtype=torch.int64, device=dev)
        p = _lib.ptr
        _lib.call("iso_meshextract_sparse_count", p(values), p(coords), p(cell_active), S, size[0], size[1], size[2], level,
                  p(self.need), p(self.totals), p(self.ws), self.ws_bytes, _lib.stream())

    def emit(self, org, spc, return_keys):
        values, coords, cell_active, S, size, level = self.args
        dev = values.device
        V, F = self.totals[:2].tolist()
        if V >= _ROW_LIMIT or F >= _ROW_LIMIT:
            raise ValueError("marching_tetrahedra_bricks: %d vertices and %d faces; the limit is 2^31 - 1 of each" % (V, F))
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        vkey = torch.empty((V,), dtype=torch.int64, device=dev) if return_keys else None
        fcell = torch.empty((F,), dtype=torch.int64, device=dev) if return_keys else None
        p = _lib.ptr
        _lib.call("iso_meshextract_sparse_emit", p(values), p(coords), p(cell_active), S, size[0], size[1], size[2], org[0],
                  org[1], org[2], spc[0], spc[1], spc[2], level, p(self.totals), p(verts) if V else None, V,
                  p(faces) if F else None, F, p(vkey) if V and return_keys else None, p(fcell) if F and return_keys else None,
                  p(self.ws), self.ws_bytes, _lib.stream())
        return (verts, faces.long(), vkey, fcell) if return_keys else (verts, faces.long())


def marching_tetrahedra_bricks(values, coords, cell_active, grid_size, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0),
                               level=0.0, return_keys=False, return_need=False):
    """marching_tetrahedra over a list of 8 x 8 x 8 bricks of grid points instead of the whole volume (include/isopoints.h
    section O): (verts (V,3) float32, faces (F,3) int64[, vert_key (V,) int64, face_cell (F,) int64][, need (S,) uint8]).

    grid_size = (nx, ny, nz), each in [2, 4096].  coords (S,3) integer: brick b holds the grid points 8 b .. 8 b + 7 per
    axis; values (S,8,8,8) float32, values[s,i,j,k] at grid point 8 coords[s] + (i,j,k) (entries outside the grid are
    ignored); cell_active (S,) bool or uint8: the cells whose lowest point lies in brick s are marched.  For every
    cell-active b all bricks b + {0,1}^3 that exist in the grid must be in the list (checked).  coords must be unique; they
    need not be sorted: the list is sorted by linear brick index (bx nby + by) nbz + bz here, and `need` comes back in the
    caller's order.

    The rule is marching_tetrahedra's.  Vertices are ordered by brick (sorted), local point, slot; faces by brick, local
    cell, tetrahedron, triangle.  vert_key = 7 p + slot and face_cell = p, p = (i ny + j) nz + k the dense linear index of
    the owning point / the cell's lowest point: sorted by them the mesh is the dense mesh of the same volume restricted to
    the cells of the cell-active bricks, bit for bit.  need[s] bit o (o = x + 2 y + 4 z in {0,1}^3): a vertex of brick s
    lies on a mesh edge that also belongs to a cell of block coords[s] - o which is not cell-active; no bit set anywhere =
    the surface does not leave the cell-active set.  Host reads: the totals, and the checks of the list.  No gradient."""
    fn = "marching_tetrahedra_bricks"
    size, org, spc, level = _grid_args(fn, grid_size, origin, spacing, level)
    if not torch.is_tensor(coords) or coords.dim() != 2 or coords.shape[1] != 3 or coords.is_floating_point():
        raise ValueError("%s: coords must be an integer tensor (S, 3)" % fn)
    S = coords.shape[0]
    if not torch.is_tensor(values) or tuple(values.shape) != (S, _BRICK, _BRICK, _BRICK):
        raise ValueError("%s: values must be (S, 8, 8, 8) for coords (S, 3)" % fn)
    if not torch.is_tensor(cell_active) or tuple(cell_active.shape) != (S,) or cell_active.is_floating_point():
        raise ValueError("%s: cell_active must be a bool or uint8 tensor (S,)" % fn)
    if S * _BRICK ** 3 >= _ROW_LIMIT:
        raise ValueError("%s: %d bricks; the limit is 2^31 - 1 grid points in all" % (fn, S))
    _on_gpu(values, coords, cell_active)
    dev = values.device
    nb = _brick_dims(size)

    def empty():
        out = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev))
        if return_keys:
            out = out + (torch.empty((0,), dtype=torch.int64, device=dev),) * 2
        return out + (torch.zeros((S,), dtype=torch.uint8, device=dev),) if return_need else out
    if S == 0:
        return empty()
    c64 = coords.long()
    lim = torch.tensor(nb, dtype=torch.int64, device=dev)
    if bool(((c64 < 0) | (c64 >= lim)).any()):
        raise ValueError("%s: coords outside the grid of %d x %d x %d bricks" % ((fn,) + tuple(nb)))
    lin, order = torch.sort(_brick_lin(c64, nb))
    if S > 1 and bool((lin[1:] == lin[:-1]).any()):
        raise ValueError("%s: coords holds a brick twice" % fn)
    active = (cell_active != 0)[order]
    want = _upper_neighbours(lin[active], nb)
    at = torch.searchsorted(lin, want).clamp(max=S - 1)
    if bool((lin[at] != want).any()):
        raise ValueError("%s: a cell-active brick lacks one of its neighbours b + {0,1}^3 in the list" % fn)
    run = _SparseCount(values.detach().float()[order].contiguous(), c64[order].int().contiguous(),
                       active.to(torch.uint8).contiguous(), size, level)
    out = run.emit(org, spc, return_keys)
    if return_need:
        need = torch.empty_like(run.need)
        need[order] = run.need
        out = out + (need,)
    return out


def _brick_points(lin, nb, size, axes, rotation, translation):
    """The sample points of the bricks `lin`: (len(lin) * 512, 3) float32, brick by brick in local order (i 8 + j) 8 + k.
    An index past the grid's end is clamped into it: its value is never looked at."""
    dev = lin.device
    b = _brick_unlin(lin, nb)
    r = torch.arange(_BRICK, device=dev)
    cols = []
    for d in range(3):
        idx = (b[:, d, None] * _BRICK + r[None]).clamp(max=size[d] - 1)             # (S, 8)
        shape = [lin.shape[0], 1, 1, 1]
        shape[d + 1] = _BRICK
        cols.append(axes[d][idx].reshape(shape).expand(-1, _BRICK, _BRICK, _BRICK))
    pts = torch.stack(cols, dim=-1).reshape(-1, 3)
    if rotation is not None:
        pts = pts @ rotation
    if translation is not None:
        pts = pts + translation
    return pts.contiguous()


def sparse_level_set(sdf, grid_size, origin=None, spacing=None, *, axes=None, band=1.5, seeds=None, rotation=None,
                     translation=None, level=0.0, max_rounds=64, return_info=False, return_keys=False,
                     _timer=None):
    """The level set {sdf = level} on a regular grid of up to 4096 points per side as (verts (V,3) float32, faces (F,3) int64
    [, vert_key (V,) int64, face_cell (F,) int64][, info]), evaluating the SDF only in 8 x 8 x 8 bricks of grid points near the surface: marching_tetrahedra_bricks on
    the bricks that a seeding finds and a closure loop completes.  Where the bricks cover the surface the mesh is
    marching_tetrahedra's on the full volume, up to the order of its vertices and faces (by brick here; return_keys gives
    marching_tetrahedra_bricks' keys to sort them back).

    Grid point (i,j,k) lies at origin + (i,j,k) * spacing in float32, or at (axes[0][i], axes[1][j], axes[2][k]) for three
    1-D float32 tensors `axes` (sdf_grid's linspace, say; they must be evenly spaced: origin and spacing, which place the
    vertices, default to axes[d][0] and the mean step).  The SDF is evaluated at point @ rotation + translation where given
    (the vertices stay in the grid's frame, as get_surface_high_res_mesh's aligned grid has it).  sdf: as sdf_grid takes it.

    Seeds.  By band: cell-block b (the cells whose lowest point has index 8 b .. 8 b + 7 per axis) is a seed iff
    |sdf(c) - level| <= band * R_b at the grid point c = min(8 b + 4, n - 1) per axis, R_b the largest distance from c to a
    corner of the block's cells; band = 1 is conservative for an exact distance, the default leaves room for a trained
    network's gradient norm, band = 0 (or None) switches it off and saves the evaluation of one point per block.  By points:
    the blocks that contain the cells of `seeds` (N,3), given in the grid's frame -- iso-points, samples of a coarse mesh.
    Closure.  The newly added bricks are evaluated, the count pass reports where the surface leaves the cell-active blocks
    (need), those blocks are added, until none is reported; so a surface component that touches one seed is extracted whole,
    whatever the SDF's Lipschitz constant.  RuntimeError after max_rounds count passes that still report a need.

    info: rounds, cell_active_bricks, sampled_bricks, seed_blocks, points_evaluated (bricks * 512 plus the band's test
    points), workspace_bytes.  Host reads: 8 bytes per round (the number of set need bits), the totals, and the sizes of the
    torch set operations on the block lists.  No gradient.  (_timer: tools/mesh_sparse_timing.py's stage clock, a callable
    name -> context manager.)"""
    fn = "sparse_level_set"
    stage = _timer if _timer is not None else (lambda name: contextlib.nullcontext())
    if axes is not None:
        if len(axes) != 3 or not all(torch.is_tensor(a) and a.dim() == 1 and a.shape[0] == int(n) for a, n in zip(axes, grid_size)):
            raise ValueError("%s: axes are three 1-D tensors of grid_size points" % fn)
        _on_gpu(*axes)
        axes = [a.detach().float().contiguous() for a in axes]
        if origin is None:
            origin = [float(a[0]) for a in axes]
        if spacing is None:
            spacing = [(float(a[-1]) - float(a[0])) / (a.shape[0] - 1) for a in axes]
    elif origin is None or spacing is None:
        raise ValueError("%s: give origin and spacing, or axes" % fn)
    size, org, spc, level = _grid_args(fn, grid_size, origin, spacing, level)
    max_rounds = int(max_rounds)
    if max_rounds < 1:
        raise ValueError("%s: max_rounds must be at least 1" % fn)
    dev = _sdf_device(sdf) if axes is None else axes[0].device
    if dev.type != "cuda":
        raise RuntimeError("iso_points_amd: the model must be on the GPU; there is no CPU path")
    if axes is None:
        o32 = torch.tensor(org, dtype=torch.float32, device=dev)
        s32 = torch.tensor(spc, dtype=torch.float32, device=dev)
        axes = [o32[d] + torch.arange(size[d], dtype=torch.float32, device=dev) * s32[d] for d in range(3)]
    if rotation is not None:
        rotation = rotation.detach().to(device=dev, dtype=torch.float32)
    if translation is not None:
        translation = translation.detach().to(device=dev, dtype=torch.float32)
    nb = _brick_dims(size)
    n_cells = [(n - 1 + _BRICK - 1) // _BRICK for n in size]          # blocks per axis that hold a cell
    evaluated = 0

    # ---- seeds: sorted linear indices of cell-blocks
    active = torch.empty((0,), dtype=torch.int64, device=dev)
    if band is not None and float(band) > 0.0:
        band = float(band)
        test, reach = [], []
        for d in range(3):
            b = torch.arange(n_cells[d], device=dev)
            c = (b * _BRICK + 4).clamp(max=size[d] - 1)
            hi = (b * _BRICK + _BRICK).clamp(max=size[d] - 1)
            test.append(axes[d][c])
            reach.append(torch.maximum(c - b * _BRICK, hi - c).double() * spc[d])
        pts = torch.stack(torch.meshgrid(*test, indexing="ij"), dim=-1).reshape(-1, 3)
        if rotation is not None:
            pts = pts @ rotation
        if translation is not None:
            pts = pts + translation
        with stage("seed"):
            f = _sdf_values(sdf, pts.contiguous()).double()
        evaluated += pts.shape[0]
        R = torch.sqrt(reach[0][:, None, None] ** 2 + reach[1][None, :, None] ** 2 + reach[2][None, None, :] ** 2).reshape(-1)
        hit = torch.nonzero((f - level).abs() <= band * R).reshape(-1)
        active = (hit // (n_cells[1] * n_cells[2]) * nb[1] + (hit // n_cells[2]) % n_cells[1]) * nb[2] + hit % n_cells[2]
    if seeds is not None:
        if not torch.is_tensor(seeds) or seeds.dim() != 2 or seeds.shape[1] != 3:
            raise ValueError("%s: seeds must be (N, 3)" % fn)
        _on_gpu(seeds)
        o64 = torch.tensor(org, dtype=torch.float64, device=dev)
        s64 = torch.tensor(spc, dtype=torch.float64, device=dev)
        cell = torch.floor((seeds.detach().double() - o64) / s64)
        top = torch.tensor([n - 2 for n in size], dtype=torch.float64, device=dev)
        cell = cell[torch.isfinite(cell).all(dim=1) & (cell >= -1).all(dim=1) & (cell <= top + 1).all(dim=1)]
        blk = torch.minimum(cell.clamp(min=0), top).long() // _BRICK
        active = torch.cat([active, (blk[:, 0] * nb[1] + blk[:, 1]) * nb[2] + blk[:, 2]])
    active = torch.unique(active)
    n_seeds = active.shape[0]
    empty = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev))
    if return_keys:
        empty = empty + (torch.empty((0,), dtype=torch.int64, device=dev),) * 2
    info = {"rounds": 0, "cell_active_bricks": 0, "sampled_bricks": 0, "seed_blocks": n_seeds, "points_evaluated": evaluated,
            "workspace_bytes": 0}
    if n_seeds == 0:
        return empty + (info,) if return_info else empty

    # ---- closure
    lin = torch.empty((0,), dtype=torch.int64, device=dev)                                # the sampled bricks, sorted
    values = torch.empty((0, _BRICK, _BRICK, _BRICK), dtype=torch.float32, device=dev)
    off = torch.tensor(_OFFSETS, dtype=torch.int64, device=dev)
    rounds = 0
    while True:
        want = _upper_neighbours(active, nb)
        fresh = want[~torch.isin(want, lin)] if lin.shape[0] else want
        if fresh.shape[0]:
            if (lin.shape[0] + fresh.shape[0]) * _BRICK ** 3 >= _ROW_LIMIT:
                raise ValueError("%s: more than 2^31 - 1 grid points in the sampled bricks" % fn)
            parts = []
            with stage("evaluate"):
                for chunk in torch.split(fresh, 32768):                                    # 16.8 M points at a time
                    parts.append(_sdf_values(sdf, _brick_points(chunk, nb, size, axes, rotation, translation)))
            evaluated += fresh.shape[0] * _BRICK ** 3
            lin, order = torch.sort(torch.cat([lin, fresh]))
            values = torch.cat([values, torch.cat(parts).reshape(-1, _BRICK, _BRICK, _BRICK)])[order].contiguous()
        S = lin.shape[0]
        flags = torch.isin(lin, active).to(torch.uint8)
        coords = _brick_unlin(lin, nb).int().contiguous()
        with stage("count"):
            run = _SparseCount(values, coords, flags, size, level)
        rounds += 1
        if int(run.totals[2]) == 0:                                                        # the round's one host read
            break
        if rounds >= max_rounds:
            raise RuntimeError("%s: the surface still leaves the cell-active blocks after %d rounds (max_rounds); %d blocks "
                               "are active" % (fn, rounds, active.shape[0]))
        more = []
        for o in range(8):
            b = coords[((run.need >> o) & 1).bool()].long() - off[o]
            more.append((b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2])
        active = torch.unique(torch.cat([active] + more))
    with stage("emit"):
        out = run.emit(org, spc, bool(return_keys))
    info.update(rounds=rounds, cell_active_bricks=int(active.shape[0]), sampled_bricks=S, points_evaluated=evaluated,
                workspace_bytes=int(run.ws_bytes))
    return out + (info,) if return_info else out


def _sdf_device(sdf):
    from .sdf_models import FusedSdf
    model = sdf.model if isinstance(sdf, FusedSdf) else sdf
    if isinstance(model, torch.nn.Module):
        for t in list(model.parameters()) + list(model.buffers()):
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _fused(sdf, device):
    """The fused evaluator of `sdf` (a FusedSdf on the SIREN or IDR kernels), or None."""
    from .sdf_models import FusedSdf, idr_spec, siren_spec
    if isinstance(sdf, FusedSdf):
        return sdf if sdf.kind in ("siren", "idr") else None
    if siren_spec(sdf) is not None or idr_spec(sdf) is not None:
        return FusedSdf(sdf, device)
    return None


def _sdf_values(sdf, pts, chunk=100000):
    """sdf at pts (n,3) -> (n,) float32: the fused value-only kernels in one launch where the model has them, any other
    callable in chunks of 100 000 points as the reference does (DSS/utils/__init__.py:575)."""
    from .sdf_models import FusedSdf
    fused = _fused(sdf, pts.device)
    if fused is not None:
        return fused(pts).reshape(-1).float()
    fn = sdf.model if isinstance(sdf, FusedSdf) else sdf
    out = []
    with torch.no_grad():
        for part in torch.split(pts, chunk, dim=0):
            val = fn(part)
            out.append(getattr(val, "sdf", val).reshape(-1).float())
    return torch.cat(out) if out else pts.new_zeros((0,))


def sdf_grid(sdf, resolution, box_side_length=2.0, points=None):
    """The SDF sampled on a grid: (values (nx,ny,nz) float32, origin, spacing), ready for marching_tetrahedra.

    Without `points` the grid is get_grid_uniform's (DSS/utils/__init__.py:554-566): resolution^3 points,
    linspace(-0.5, 0.5, resolution) * box_side_length along every axis, values[i,j,k] = sdf(x_i, y_j, z_k); origin and
    spacing are three floats each.  With `points` (nx,ny,nz,3) the SDF is evaluated there -- a rotated grid, say -- and
    origin and spacing are None: the caller made the grid and knows its frame.

    sdf: a FusedSdf, or a model that siren_spec / idr_spec accept, runs on the fused value-only kernels in one launch; any
    other callable (points (n,3) -> values, or an object with .sdf) is called on chunks of 100 000 points."""
    fn = "sdf_grid"
    if points is not None:
        if not torch.is_tensor(points) or points.dim() != 4 or points.shape[-1] != 3:
            raise ValueError("%s: points must be (nx, ny, nz, 3)" % fn)
        _on_gpu(points)
        pts = points.detach().float().reshape(-1, 3).contiguous()
        return _sdf_values(sdf, pts).reshape(points.shape[:3]), None, None
    n = int(resolution)
    if n < 2:
        raise ValueError("%s: resolution must be at least 2" % fn)
    dev = _sdf_device(sdf)
    if dev.type != "cuda":
        raise RuntimeError("iso_points_amd: the model must be on the GPU; there is no CPU path")
    axis64 = np.linspace(-0.5, 0.5, n) * float(box_side_length)
    axis = torch.from_numpy(axis64.astype(np.float32)).to(dev)
    pts = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    origin, spacing = (float(axis64[0]),) * 3, (float(axis64[1] - axis64[0]),) * 3
    return _sdf_values(sdf, pts).reshape(n, n, n), origin, spacing


def mesh_components(verts, faces):
    """Connected components of a mesh over shared vertex indices, what trimesh's split(only_watertight=False) groups by
    (DSS/utils/__init__.py:595, :651): (labels (F,) int64, areas (C,) float64).  Components are numbered by their lowest
    vertex index; areas[c] is the float64 sum of the face areas of component c, in face order.  Plain torch on the tensors'
    device: minimum-label hooking with pointer jumping, one host read per round (a few rounds), and one for C."""
    fn = "mesh_components"
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[-1] != 3:
        raise ValueError("%s: verts must be (V, 3)" % fn)
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[-1] != 3 or faces.is_floating_point():
        raise ValueError("%s: faces must be an integer tensor (F, 3)" % fn)
    faces = faces.long()
    dev = faces.device
    if faces.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.float64, device=dev)
    u = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2], faces[:, 1], faces[:, 2], faces[:, 0]])
    v = torch.cat([faces[:, 1], faces[:, 2], faces[:, 0], faces[:, 0], faces[:, 1], faces[:, 2]])
    parent = torch.arange(verts.shape[0], dtype=torch.int64, device=dev)
    while True:
        # parent[x] <= x always.  At a fixed point every parent is a root and equal across every edge: the component's
        # lowest vertex
        grand = parent[parent]
        nxt = parent.scatter_reduce(0, parent[u], grand[v], "amin")      # hook the parent ...
        nxt = nxt.scatter_reduce(0, u, grand[v], "amin")                 # ... and the vertex to the neighbour's grandparent
        nxt = torch.minimum(nxt, grand)                                   # pointer jumping
        if torch.equal(nxt, parent):
            break
        parent = nxt
    _roots, labels = torch.unique(parent[faces[:, 0]], return_inverse=True)
    tri = verts.detach().double()[faces]
    area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1)
    order = torch.argsort(labels, stable=True)
    run = torch.cat([area.new_zeros(1), torch.cumsum(area[order], 0)])    # a scan, not atomics: the same bits every run
    size = torch.bincount(labels)
    ends = torch.cumsum(size, 0)
    return labels, run[ends] - run[ends - size]


def _largest(verts, faces):
    labels, areas = mesh_components(verts, faces)
    if areas.numel() == 0:
        return verts[:0], faces.long()[:0]
    kept = faces.long()[labels == areas.argmax()]
    used = torch.zeros((verts.shape[0],), dtype=torch.bool, device=verts.device)
    used[kept.reshape(-1)] = True
    return verts[used], (torch.cumsum(used, 0) - 1)[kept]


def largest_component(verts, faces):
    """(verts, faces) of the component of largest area (the first of equals), as the reference keeps
    components[areas.argmax()] (DSS/utils/__init__.py:595-597, :650-653): vertices that no kept face uses are dropped and
    the faces re-indexed; the order of what stays is unchanged."""
    return _largest(verts, faces)


def _sdf_normals(sdf, verts):
    """Unit SDF gradients at verts: the fused gradient kernel where the model has one, autograd otherwise."""
    from .sdf_models import FusedSdf, idr_sdf_and_grad, siren_sdf_and_grad
    fused = _fused(sdf, verts.device)
    if fused is not None:
        grad_fn = siren_sdf_and_grad if fused.kind == "siren" else idr_sdf_and_grad
        grad = grad_fn(fused.model, verts, need_grad=True, packed=fused.packed)[1]
    else:
        fn = sdf.model if isinstance(sdf, FusedSdf) else sdf
        grads = []
        for part in torch.split(verts.detach(), 100000, dim=0):
            with torch.enable_grad():
                x = part.clone().requires_grad_(True)
                val = fn(x)
                grads.append(torch.autograd.grad(getattr(val, "sdf", val).sum(), x)[0])
        grad = torch.cat(grads) if grads else verts.new_zeros((0, 3))
    return grad / grad.norm(dim=-1, keepdim=True).clamp_min(1e-30)


def _aligned_grid(lo, hi, resolution):
    """get_grid (DSS/utils/__init__.py:658-696) from the bounding box of the aligned samples: `resolution` points along the
    shortest axis over [min - 0.2, max + 0.2], the same step along the other two.  (origin (3,), step, sizes (3,))"""
    eps = 0.2
    short = int(np.argmin(hi - lo))
    axis = np.linspace(lo[short] - eps, hi[short] + eps, resolution)
    step = (axis.max() - axis.min()) / (resolution - 1)
    sizes = [resolution if d == short else len(np.arange(lo[d] - eps, hi[d] + step + eps, step)) for d in range(3)]
    return lo - eps, float(step), sizes


def get_surface_high_res_mesh(sdf, resolution=100, box_side_length=2.0, largest_component=True, return_normals=False,
                              generator=None, sparse=False, texture=None, texture_kwargs=None):
    """The SDF's zero level set as a mesh, by the steps of the reference's get_surface_high_res_mesh
    (DSS/utils/__init__.py:569-655): a 64^3 mesh over the box -> its largest component -> 10 000 surface samples
    (sample_points_from_meshes, seeded through `generator`) -> their PCA frame -> the aligned grid of get_grid with
    `resolution` points along its shortest side -> the extraction on that grid -> rotated back -> the largest component.

    Returns (verts (V,3) float32, faces (F,3) int64) on the model's device, with return_normals also the unit SDF gradient
    at every vertex (V,3); tensors, not a trimesh object, and empty ones where the SDF has no sign change on a grid (the
    reference returns an empty Trimesh).  Not the reference's triangles: marching_tetrahedra is not Lewiner's marching
    cubes; the PCA axes come in ascending order of variance; normals are SDF gradients, not skimage's volume gradients.
    Host reads: the totals of both extractions, the component rounds, the 3 x 3 covariance and the samples' bounding box.

    sparse=True takes the second extraction through sparse_level_set on the same aligned grid, seeded by band and by the
    10 000 samples: the SDF is evaluated near the surface only and `resolution` may go past marching_tetrahedra's 1024
    points per side, up to 4096 on the longest side.  The default is the dense path, unchanged.

    texture: a texture.NeuralTexture; the result then ends with the vertex colours (V,3) in [0, 1] of texture.vertex_colors
    (Generator.estimate_colors, implicit_modeling.py:790-820, which gives generate_mesh its colours); texture_kwargs go to
    that call (c, with_normals, camera_centers).  The default, None, returns what it always did."""
    keep_largest, res = bool(largest_component), int(resolution)
    if res < 2:
        raise ValueError("get_surface_high_res_mesh: resolution must be at least 2")

    def result(verts, faces):
        out = (verts, faces, _sdf_normals(sdf, verts)) if return_normals else (verts, faces)
        if texture is not None:
            from .texture import vertex_colors
            out = out + (vertex_colors(sdf, texture, verts, **(texture_kwargs or {})),)
        return out
    values, origin, spacing = sdf_grid(sdf, 64, box_side_length)
    verts, faces = marching_tetrahedra(values, origin, spacing)
    if faces.shape[0] == 0:
        return result(verts, faces)
    verts, faces = _largest(verts, faces)
    cloud = sample_points_from_meshes((verts[None], faces[None]), 10000, generator=generator)[0]
    mean = cloud.mean(dim=0)
    centred = cloud - mean
    cov = (centred.t() @ centred).double().cpu()
    vecs = torch.linalg.eigh(cov)[1].t().contiguous()                     # rows: the axes, ascending variance
    if torch.det(vecs) < 0:
        vecs = vecs[[0, 2, 1]]
    vecs = vecs.to(device=cloud.device, dtype=torch.float32)
    aligned = centred @ vecs.t()
    box = torch.stack([aligned.amin(dim=0), aligned.amax(dim=0)]).double().cpu().numpy()
    lo, step, sizes = _aligned_grid(box[0], box[1], res)
    axes = [torch.from_numpy((lo[d] + step * np.arange(sizes[d])).astype(np.float32)).to(cloud.device) for d in range(3)]
    if sparse:
        verts, faces = sparse_level_set(sdf, sizes, [float(x) for x in lo], (step,) * 3, axes=axes, seeds=aligned,
                                        rotation=vecs, translation=mean)
    else:
        grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
        values = sdf_grid(sdf, None, points=grid @ vecs + mean)[0]
        verts, faces = marching_tetrahedra(values, [float(x) for x in lo], (step,) * 3)
    verts = verts @ vecs + mean
    if keep_largest:
        verts, faces = _largest(verts, faces)
    return result(verts, faces)
