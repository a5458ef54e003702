"""Mesh rasterisation: pytorch3d.renderer's rasterize_meshes / MeshRasterizer / HardFlatShader as the reference calls them
(scripts/create_mvr_data_from_mesh.py:143-216, the synthetic training sets; DSS/training/losses.py:550-578, the depth
layers of SignedDistanceLoss; tests/test_data.py and tests/test_dvr_camera.py): per pixel the K nearest faces with depth,
barycentric coordinates and the negative squared distance to the face's outline.

The rasteriser is the HIP kernel of csrc/mesh_raster.hip (include/isopoints.h section M states the rule); there is no CPU
path.  blur_radius is always 0 in the reference and nothing else is accepted.  There is no backward pass: both call sites
run without gradients, the inputs are detached and no output ever requires grad.

hard_flat_shading and render_views are plain torch on whatever device the fragments live on.
"""
from collections import namedtuple

import torch

from . import _lib
from .loss import _on_gpu, _packed_mesh

Fragments = namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords", "dists"])
RenderedViews = namedtuple("RenderedViews", ["images", "mask", "depth", "fragments"])

_LIMIT = 2 ** 31
MAX_FACES_PER_PIXEL = 8


class RasterizationSettings:
    """pytorch3d.renderer.RasterizationSettings with the fields rasterize_meshes takes.  bin_size and max_faces_per_bin are
    kept for signature compatibility and have no effect on the result."""

    def __init__(self, image_size=256, blur_radius=0.0, faces_per_pixel=1, bin_size=None, max_faces_per_bin=None,
                 perspective_correct=False, cull_backfaces=False):
        self.image_size = image_size
        self.blur_radius = blur_radius
        self.faces_per_pixel = faces_per_pixel
        self.bin_size = bin_size
        self.max_faces_per_bin = max_faces_per_bin
        self.perspective_correct = perspective_correct
        self.cull_backfaces = cull_backfaces


def _check_settings(fn, image_size, blur_radius, faces_per_pixel):
    """(S, K) of the arguments, or ValueError."""
    if isinstance(blur_radius, bool) or not isinstance(blur_radius, (int, float)) or float(blur_radius) != 0.0:
        raise ValueError("%s: blur_radius must be 0.0 (the reference passes nothing else), got %r" % (fn, blur_radius))
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2 or image_size[0] != image_size[1]:
            raise ValueError("%s: only square images, got image_size %r" % (fn, image_size))
        image_size = image_size[0]
    if isinstance(image_size, bool) or not isinstance(image_size, int) or image_size < 1:
        raise ValueError("%s: image_size must be a positive integer, got %r" % (fn, image_size))
    K = faces_per_pixel
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= MAX_FACES_PER_PIXEL:
        raise ValueError("%s: faces_per_pixel must be an integer in 1..%d, got %r" % (fn, MAX_FACES_PER_PIXEL, K))
    return image_size, K


def _mesh_lengths(meshes, first, T, fn):
    """num_faces_per_mesh (N,) int64 beside first_idx."""
    if hasattr(meshes, "num_faces_per_mesh"):
        num = meshes.num_faces_per_mesh()
        if not torch.is_tensor(num) or num.dim() != 1 or num.is_floating_point() or num.shape[0] != first.shape[0]:
            raise ValueError("%s: num_faces_per_mesh must be an integer tensor of shape (N,)" % fn)
        return num.to(dtype=torch.int64)
    first = first.to(dtype=torch.int64)
    end = torch.full((1,), T, dtype=torch.int64, device=first.device)
    return torch.cat([first[1:], end]) - first


def _raster_packed(tris, first, num, S, K, perspective_correct, cull_backfaces, timings=None):
    """The three passes on packed float32 triangles (F,3,3) in NDC with view z, first / num (N,) int64, all on the GPU.
    timings: a dict that receives torch events around the passes (tools/mesh_raster_timing.py)."""
    dev, N, F = tris.device, first.shape[0], tris.shape[0]
    i64 = torch.empty((N, S, S, K), dtype=torch.int64, device=dev)
    zbuf = torch.empty((N, S, S, K), dtype=torch.float32, device=dev)
    bary = torch.empty((N, S, S, K, 3), dtype=torch.float32, device=dev)
    dists = torch.empty((N, S, S, K), dtype=torch.float32, device=dev)
    if N == 0:
        return Fragments(i64, zbuf, bary, dists)
    lib = _lib.load()
    T = lib.iso_splat_tiles_per_side(S)
    ntiles = N * T * T
    p, s = _lib.ptr, _lib.stream()
    tile_cnt = torch.zeros((ntiles + 1,), dtype=torch.int32, device=dev)
    tile_off = torch.empty((ntiles + 1,), dtype=torch.int32, device=dev)
    cursor = torch.empty((ntiles + 1,), dtype=torch.int32, device=dev)
    cull, persp = int(bool(cull_backfaces)), int(bool(perspective_correct))

    def mark(name):
        if timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            timings[name] = ev

    mark("begin")
    _lib.call("iso_meshraster_count", p(tris), p(first), p(num), N, F, S, cull, p(tile_cnt), s)
    _lib.call("iso_splat_tile_offsets", p(tile_cnt), p(tile_off), p(cursor), ntiles + 1, s)
    mark("count")
    total = int(tile_off[ntiles].item())                 # the one host read: the size of the pair list
    if total < 0:
        raise RuntimeError("rasterize_meshes: more than 2^31 - 1 (face, tile) pairs")
    pairs = torch.empty((total,), dtype=torch.int32, device=dev) if total else None
    mark("read")
    _lib.call("iso_meshraster_fill", p(tris), p(first), p(num), N, F, S, cull, p(cursor), p(tile_off), p(pairs), total, s)
    mark("fill")
    _lib.call("iso_meshraster_pixels", p(tris), N, F, S, K, persp, p(tile_off), p(pairs), total, p(i64), p(zbuf), p(bary),
              p(dists), s)
    mark("raster")
    if timings is not None:
        timings["pairs"] = total
    return Fragments(i64, zbuf, bary, dists)


def rasterize_meshes(meshes, image_size=256, blur_radius=0.0, faces_per_pixel=8, bin_size=None, max_faces_per_bin=None,
                     perspective_correct=False, cull_backfaces=False):
    """pytorch3d.renderer.mesh.rasterize_meshes at blur_radius = 0: Fragments(pix_to_face (N,S,S,K) int64, zbuf (N,S,S,K),
    bary_coords (N,S,S,K,3), dists (N,S,S,K)) float32, -1 in every empty slot.

    `meshes` is a pytorch3d-style Meshes (verts_packed / faces_packed / mesh_to_faces_packed_first_idx /
    num_faces_per_mesh) or the (verts (N,V,3), faces (N,F,3)[, num_faces]) tuple ops.sample_points_from_meshes takes, its
    vertices already in NDC (+X left, +Y up) with the view-space depth as z -- what MeshRasterizer.transform returns.
    pix_to_face indexes the packed faces.  Per pixel the faces_per_pixel (1..8) nearest faces in ascending (depth, face
    index) order; the rule, bit for bit, is include/isopoints.h section M.  Differences from pytorch3d: faces with |area| <=
    1e-8 or a non-finite coordinate are skipped instead of damped by an epsilon, and a face list cannot overflow.

    bin_size and max_faces_per_bin are accepted for signature compatibility and have no effect on the result.  blur_radius
    must be 0.0.  No backward pass: the inputs are detached and the outputs never require grad.  One host read (4 bytes,
    the size of the face-tile pair list) per call.  Limits, refused: N * S * S * K < 2^31, fewer than 2^31 packed faces."""
    fn = "rasterize_meshes"
    S, K = _check_settings(fn, image_size, blur_radius, faces_per_pixel)
    tris, first = _packed_mesh(meshes, fn)
    if not torch.is_tensor(first) or first.dim() != 1 or first.is_floating_point():
        raise ValueError("%s: mesh_to_faces_packed_first_idx must be an integer tensor of shape (N,)" % fn)
    if not tris.is_floating_point():
        raise ValueError("%s: vertices must be floating point" % fn)
    N, F = first.shape[0], tris.shape[0]
    num = _mesh_lengths(meshes, first, F, fn)
    if F >= _LIMIT:
        raise ValueError("%s: %d packed faces; the limit is 2^31 - 1" % (fn, F))
    if N * S * S * K >= _LIMIT:
        raise ValueError("%s: %d meshes x %d^2 pixels x %d faces per pixel; the limit is 2^31 - 1 slots" % (fn, N, S, K))
    _on_gpu(tris)
    dev = tris.device
    return _raster_packed(tris.detach().float().contiguous(), first.to(device=dev, dtype=torch.int64).contiguous(),
                          num.to(device=dev, dtype=torch.int64).contiguous(), S, K, perspective_correct, cull_backfaces)


def _camera_matrices(cameras):
    """(views, projs), each (N,4,4): SurfaceSplatting._camera_matrices."""
    from .rasterizer import SurfaceSplatting
    views, projs = SurfaceSplatting._camera_matrices(cameras)
    if (not torch.is_tensor(views) or not torch.is_tensor(projs) or views.dim() != 3 or views.shape[1:] != (4, 4)
            or projs.shape != views.shape):
        raise ValueError("MeshRasterizer: cameras must give views and projs of shape (N, 4, 4)")
    return views, projs


class MeshRasterizer:
    """pytorch3d.renderer.MeshRasterizer: world-space meshes seen through cameras -> Fragments.

    cameras: (views, projs), each (N,4,4) in pytorch3d's row-vector convention (projs the full world -> NDC matrix), or a
    camera object with get_world_to_view_transform() / get_full_projection_transform(); given at construction or per call.
    One mesh with N cameras is extended to N views, B > 1 meshes need B cameras.  The transform is pytorch3d's, in torch:
    [v, 1] @ view for the depth, [v, 1] @ proj with the homogeneous divide for x and y.  A Meshes object of B > 1 meshes
    costs one host read of its face counts."""

    def __init__(self, cameras=None, raster_settings=None):
        self.cameras = cameras
        self.raster_settings = raster_settings if raster_settings is not None else RasterizationSettings()

    def to(self, device):
        return self

    def transform(self, meshes_world, cameras=None):
        """(face_verts (F',3,3) in NDC with view z, first_idx (N,), num_faces (N,), world triangles (F',3,3)) of the N views."""
        fn = "MeshRasterizer"
        cameras = cameras if cameras is not None else self.cameras
        if cameras is None:
            raise ValueError("%s: cameras must be given at construction or in the call" % fn)
        views, projs = _camera_matrices(cameras)
        tris, first = _packed_mesh(meshes_world, fn)
        if not tris.is_floating_point():
            raise ValueError("%s: vertices must be floating point" % fn)
        B, N, F, dev = first.shape[0], views.shape[0], tris.shape[0], tris.device
        if B == 1:
            tris = tris[None].expand(N, F, 3, 3).reshape(N * F, 3, 3)
            counts = [F] * N
        elif B == N:
            counts = [int(c) for c in _mesh_lengths(meshes_world, first, F, fn).tolist()]
        else:
            raise ValueError("%s: %d meshes and %d cameras: one mesh or one per camera" % (fn, B, N))
        num = torch.tensor(counts, dtype=torch.int64, device=dev)
        first = torch.cumsum(num, 0) - num
        view_of = torch.repeat_interleave(torch.arange(N, device=dev), num, output_size=sum(counts))
        tris = tris.detach().float()
        hom = torch.cat([tris, torch.ones_like(tris[..., :1])], dim=-1)                      # (F',3,4)
        pv = torch.bmm(hom, views.to(dev).float()[view_of])
        pn = torch.bmm(hom, projs.to(dev).float()[view_of])
        ndc = torch.cat([pn[..., :2] / pn[..., 3:4], pv[..., 2:3]], dim=-1).contiguous()
        return ndc, first, num, tris

    def __call__(self, meshes_world, cameras=None, **kwargs):
        fn = "MeshRasterizer"
        rs = kwargs.get("raster_settings", self.raster_settings)
        S, K = _check_settings(fn, rs.image_size, rs.blur_radius, rs.faces_per_pixel)
        ndc, first, num, _ = self.transform(meshes_world, cameras)
        N, F = first.shape[0], ndc.shape[0]
        if F >= _LIMIT or N * S * S * K >= _LIMIT:
            raise ValueError("%s: %d faces, %d views x %d^2 pixels x %d faces per pixel; the limits are 2^31 - 1" % (fn, F, N, S, S, K))
        _on_gpu(ndc)
        return _raster_packed(ndc, first, num, S, K, rs.perspective_correct, rs.cull_backfaces)

    forward = __call__


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-6)


def hard_flat_shading(fragments, face_verts_world, camera_position, light_direction=None, light_location=None,
                      ambient=0.5, diffuse=0.3, specular=0.2, shininess=64, face_colors=None, background=(1.0, 1.0, 1.0)):
    """pytorch3d's HardFlatShader for one directional or one point light -> images (N,S,S,4), alpha = coverage.

    fragments: rasterize_meshes' result; face_verts_world (F,3,3): the packed faces' world-space vertices in the order
    pix_to_face indexes; camera_position (N,3) or (3,).  Exactly one of light_direction (towards the light) and
    light_location, each (3,) or (N,3); neither: the direction (0, 1, 0), pytorch3d's default.  face_colors (F,3,3): rgb
    per face vertex, interpolated with bary_coords (None: white).
    n = normalize(cross(v1 - v0, v2 - v0)); p = the bary_coords-weighted world vertices; l the unit direction to the light;
    colour = (ambient + diffuse relu(n . l)) texel + specular relu(v . r)^shininess [n . l > 0], r = -l + 2 (n . l) n,
    v the unit direction to the camera.  Hard blend: slot 0 where covered, `background` elsewhere.  Plain torch."""
    if light_direction is not None and light_location is not None:
        raise ValueError("hard_flat_shading: give light_direction or light_location, not both")
    p2f, bary = fragments.pix_to_face[..., 0], fragments.bary_coords[..., 0, :]
    if face_verts_world.dim() != 3 or face_verts_world.shape[1:] != (3, 3):
        raise ValueError("hard_flat_shading: face_verts_world must be (F, 3, 3)")
    N = p2f.shape[0]
    dt, dev = face_verts_world.dtype, face_verts_world.device
    covered = p2f >= 0
    idx = p2f.clamp_min(0)
    fv = face_verts_world[idx] if face_verts_world.shape[0] else face_verts_world.new_zeros(p2f.shape + (3, 3))
    bary = bary.to(dt)
    normal = _unit(torch.cross(fv[..., 1, :] - fv[..., 0, :], fv[..., 2, :] - fv[..., 0, :], dim=-1))
    point = (bary[..., None] * fv).sum(-2)
    texel = torch.ones_like(point)
    if face_colors is not None:
        if face_colors.shape != face_verts_world.shape:
            raise ValueError("hard_flat_shading: face_colors must be (F, 3, 3) like face_verts_world")
        texel = (bary[..., None] * face_colors.to(dt)[idx]).sum(-2)

    def per_view(v):
        v = torch.as_tensor(v, dtype=dt, device=dev)
        return v.reshape(-1, 1, 1, 3).expand(N, 1, 1, 3) if v.numel() == 3 else v.reshape(N, 1, 1, 3)

    if light_location is not None:
        light = _unit(per_view(light_location) - point)
    else:
        light = _unit(per_view(light_direction if light_direction is not None else (0.0, 1.0, 0.0))).expand_as(point)
    cos = (normal * light).sum(-1, keepdim=True)
    view = _unit(per_view(camera_position) - point)
    reflect = -light + 2.0 * cos * normal
    spec = torch.relu((view * reflect).sum(-1, keepdim=True)) * (cos > 0).to(dt)
    colour = (ambient + diffuse * torch.relu(cos)) * texel + specular * spec ** shininess
    bg = torch.as_tensor(background, dtype=dt, device=dev).expand_as(colour)
    rgb = torch.where(covered[..., None], colour, bg)
    return torch.cat([rgb, covered[..., None].to(dt)], dim=-1)


def render_views(meshes_world, cameras, image_size=256, faces_per_pixel=5, zfar=100.0, perspective_correct=False,
                 cull_backfaces=False, fragments=None, face_verts_world=None, **shading):
    """What scripts/create_mvr_data_from_mesh.py:204-216 saves per view: RenderedViews(images (N,S,S,4) RGBA with the mask
    as alpha, mask (N,S,S,1) uint8 0 / 255, depth (N,S,S,1) = where(mask, zbuf[..., :1], zfar), fragments).

    meshes_world / cameras as MeshRasterizer takes them; zfar a float or one per view.  **shading goes to
    hard_flat_shading (lights, material, face_colors, background); the camera position is read off the view matrices.
    With `fragments` and `face_verts_world` given (any device) nothing is rasterised: shading and masks only."""
    views, _ = _camera_matrices(cameras)
    if fragments is None:
        rast = MeshRasterizer(cameras, RasterizationSettings(image_size=image_size, faces_per_pixel=faces_per_pixel,
                                                             perspective_correct=perspective_correct,
                                                             cull_backfaces=cull_backfaces))
        S, K = _check_settings("render_views", image_size, 0.0, faces_per_pixel)
        ndc, first, num, face_verts_world = rast.transform(meshes_world)
        if ndc.shape[0] >= _LIMIT or first.shape[0] * S * S * K >= _LIMIT:
            raise ValueError("render_views: the limits are 2^31 - 1 faces and output slots")
        _on_gpu(ndc)
        fragments = _raster_packed(ndc, first, num, S, K, perspective_correct, cull_backfaces)
    elif face_verts_world is None:
        raise ValueError("render_views: fragments need the face_verts_world they index")
    dev = fragments.pix_to_face.device
    cam = torch.linalg.inv(views.to(dev).to(face_verts_world.dtype))[:, 3, :3]
    images = hard_flat_shading(fragments, face_verts_world.to(dev), cam, **shading)
    mask = fragments.pix_to_face[..., :1] >= 0
    far = torch.as_tensor(zfar, dtype=fragments.zbuf.dtype, device=dev).reshape(-1, 1, 1, 1).expand_as(mask)
    depth = torch.where(mask, fragments.zbuf[..., :1], far)
    return RenderedViews(images, mask.to(torch.uint8) * 255, depth, fragments)
