"""sha256 of every gradient the three fused backward passes write, from seeded inputs, through the C ABI: one line per
case, `family case tensor:hash ...`.  Two builds of the library compute the same bits when their outputs are the same text:

    python tools/grad_bits.py texture > new.txt;  ISO_DEV_LIB=/path/to/other/libisopoints_hip.so python tools/grad_bits.py texture > old.txt

The cases sit on the edges of the planned reduction (csrc/grad_sums.h): one point, fewer rows than a 16-row group, one past
a chunk of points, one past a workspace chunk.  The weights are a seeded raw vector, not a fitted network: the sums are the
same arithmetic.  The gradient of the raw vector is hashed per layer (weight, bias), the inputs' gradients each.
usage: python tools/grad_bits.py [texture] [siren] [idr]   (no family: all three)"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iso_points_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")


def h16(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def layers(g_raw, sizes):
    """[(name, rows, cols)] -> 'name.w:hash name.b:hash' over the raw layout W | b per layer"""
    out, at = [], 0
    for name, rows, cols in sizes:
        out.append("%s.w:%s" % (name, h16(g_raw[at:at + rows * cols])))
        at += rows * cols
        out.append("%s.b:%s" % (name, h16(g_raw[at:at + rows])))
        at += rows
    assert at == g_raw.numel(), (at, g_raw.numel())
    return out


def texture():
    lib = _lib.load()
    for shape in ((256, 2, 30, 6, 4), (512, 2, 31, 6, 4)):
        H, NL, C, G, Fq = shape
        D0 = C + G + (3 + 6 * Fq if Fq >= 0 else 0)
        for n in (1, 63, 513, 20001):
            gen = torch.Generator().manual_seed(1000 * H + n)
            raw = rand(gen, lib.iso_texture_raw_floats(*shape), scale=0.05)
            pts, nrm, codes = rand(gen, n, 3), torch.nn.functional.normalize(rand(gen, n, 3), dim=-1), rand(gen, n, C)
            cams = rand(gen, 2, 3, scale=3.0)
            origin_of = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int32).to(DEV)
            g = rand(gen, n, 3)
            packed_fw = torch.empty(lib.iso_texture_packed_floats(*shape), device=DEV)
            packed_bw = torch.empty(lib.iso_texgrad_packed_floats(*shape), device=DEV)
            _lib.call("iso_texture_pack_weights", _lib.ptr(raw), _lib.ptr(packed_fw), *shape, _lib.stream())
            _lib.call("iso_texgrad_pack_weights", _lib.ptr(raw), _lib.ptr(packed_bw), *shape, _lib.stream())
            g_raw, g_pts, g_nrm, g_codes = nan(raw.numel()), nan(n, 3), nan(n, 3), nan(n, C)
            ws = torch.empty(lib.iso_texgrad_workspace_bytes(n, *shape), dtype=torch.uint8, device=DEV)
            _lib.call("iso_texgrad_backward", _lib.ptr(pts), _lib.ptr(nrm), _lib.ptr(codes), _lib.ptr(cams), _lib.ptr(origin_of), 2,
                      _lib.ptr(g), n, _lib.ptr(packed_fw), _lib.ptr(packed_bw), *shape, _lib.ptr(g_raw), _lib.ptr(g_pts),
                      _lib.ptr(g_nrm), _lib.ptr(g_codes), _lib.ptr(ws), ws.numel(), _lib.stream())
            torch.cuda.synchronize()
            assert all(torch.isfinite(t).all() for t in (g_raw, g_pts, g_nrm, g_codes)) and g_raw.abs().max() > 0, (shape, n)
            sizes = [("lin%d" % l, H, D0 if l == 0 else H) for l in range(NL)] + [("head", 3, H)]
            print("texture %s n=%d" % (shape, n), "points:" + h16(g_pts), "normals:" + h16(g_nrm), "codes:" + h16(g_codes),
                  *layers(g_raw, sizes), flush=True)


def siren_raw(gen, H, L, width):
    """raw vector of an H-wide network whose rows and columns at or past `width` are zero (a narrower network, padded)"""
    keep = (torch.arange(H) < width).float()
    parts = [torch.randn(H, 3, generator=gen) * keep[:, None], torch.randn(H, generator=gen) * 0.1 * keep]
    for _ in range(L):
        parts += [torch.randn(H, H, generator=gen) * (6.0 / H) ** 0.5 / 30.0 * keep[:, None] * keep[None, :],
                  torch.randn(H, generator=gen) * 0.01 * keep]
    parts += [torch.randn(H, generator=gen) * 0.1 * keep, torch.randn(1, generator=gen)]
    return torch.cat([p.reshape(-1) for p in parts]).to(DEV)


def siren():
    lib = _lib.load()
    for H, width, tail in ((64, 64, False), (128, 128, False), (256, 256, False), (64, 48, False), (128, 128, True)):
        for L in (0, 3, 8):
            for with_v in (True, False):
                for n in (1, 33, 257, 16385):
                    gen = torch.Generator().manual_seed(100000 * H + 1000 * L + n + width)
                    raw = siren_raw(gen, H, L, width)
                    assert raw.numel() == lib.iso_siren_raw_floats(H, L)
                    packed = torch.empty(lib.iso_siren_packed_floats(H, L), device=DEV)
                    _lib.call("iso_siren_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, L, _lib.stream())
                    pts, u = rand(gen, n, 3, scale=0.5), rand(gen, n)
                    v = rand(gen, n, 3) if with_v else None
                    b0_tail = rand(gen, H, scale=1e-4) if tail else None
                    g_raw, g_pts = nan(raw.numel()), nan(n, 3)
                    ws = torch.empty(lib.iso_sirengrad_workspace_bytes(n, H, L), dtype=torch.uint8, device=DEV)
                    args = (_lib.ptr(pts), _lib.ptr(u), _lib.ptr(v), n, _lib.ptr(raw), _lib.ptr(packed), H, L, 30.0, 30.0,
                            _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(ws), ws.numel(), _lib.stream())
                    if tail:
                        _lib.call("iso_sirengrad_backward_b0", *args, _lib.ptr(b0_tail))
                    else:
                        _lib.call("iso_sirengrad_backward", *args)
                    torch.cuda.synchronize()
                    assert torch.isfinite(g_raw).all() and torch.isfinite(g_pts).all() and g_raw.abs().max() > 0, (H, L, n)
                    sizes = [("lin0", H, 3)] + [("lin%d" % l, H, H) for l in range(1, L + 1)] + [("head", 1, H)]
                    print("siren H=%d width=%d L=%d v=%d b0_tail=%d n=%d" % (H, width, L, with_v, tail, n), "points:" + h16(g_pts),
                          *layers(g_raw, sizes), flush=True)


def idr():
    lib = _lib.load()
    for H, NL, skip, NF in ((128, 3, 1, 4), (256, 4, 2, 6), (512, 2, -1, 6)):
        D0 = 3 + 6 * NF
        for with_v in (True, False):
            for n in (1, 257, 8193):
                gen = torch.Generator().manual_seed(100000 * H + 1000 * NL + n)
                raw = rand(gen, lib.iso_idr_raw_floats(H, NL, skip, NF), scale=0.05)
                packed = torch.empty(lib.iso_idr_packed_floats(H, NL), device=DEV)
                _lib.call("iso_idr_pack_weights", _lib.ptr(raw), _lib.ptr(packed), H, NL, skip, NF, _lib.stream())
                pts, u = rand(gen, n, 3, scale=0.5), rand(gen, n)
                v = rand(gen, n, 3) if with_v else None
                g_raw, g_pts = nan(raw.numel()), nan(n, 3)
                ws = torch.empty(lib.iso_idrgrad_workspace_bytes(n, H, NL, skip, NF), dtype=torch.uint8, device=DEV)
                _lib.call("iso_idrgrad_backward", _lib.ptr(pts), _lib.ptr(u), _lib.ptr(v), n, _lib.ptr(raw), _lib.ptr(packed), H, NL,
                          skip, NF, 100.0, _lib.ptr(g_raw), _lib.ptr(g_pts), _lib.ptr(ws), ws.numel(), _lib.stream())
                torch.cuda.synchronize()
                assert torch.isfinite(g_raw).all() and torch.isfinite(g_pts).all() and g_raw.abs().max() > 0, (H, NL, skip, n)
                sizes = [("lin%d" % l, H - D0 if (skip >= 1 and l == skip - 1) else H, D0 if l == 0 else H) for l in range(NL)]
                print("idr %s v=%d n=%d" % ((H, NL, skip, NF), with_v, n), "points:" + h16(g_pts),
                      *layers(g_raw, sizes + [("head", 1, H)]), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("tools/grad_bits.py needs the GPU")
    families = {"texture": texture, "siren": siren, "idr": idr}
    print("library:", _lib.LIB_PATH, file=sys.stderr)
    for name in (sys.argv[1:] or list(families)):
        families[name]()
