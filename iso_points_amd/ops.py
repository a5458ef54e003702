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
"""
import math

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
