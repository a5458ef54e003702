"""The on-chip form of the split-fp16 SIREN gradient step (iso_siren_set_step_form(1): four waves of 512 registers, the
derivative stash in LDS and registers) against the eight-wave form with the global stash (form 0): bit for bit."""
import pytest
import torch

from util import sphere_cloud

pytestmark = pytest.mark.gpu

# 24 609 = 256 * 96 + 33: a workgroup takes a second tile, the drawn-tile counter runs, both tile shapes serve one list;
# 60 000: several rounds
SIZES = (1, 31, 32, 33, 95, 96, 97, 197, 24609, 60000)
T = 10
_models = {}


def _siren(dev, L, fitted):
    """chaotic: default-initialised, omega = 30 (lists stay long); fitted: to the unit sphere, as bench.py: fitted_siren"""
    key = (L, fitted)
    if key not in _models:
        from iso_points_amd.sdf_models import Siren
        torch.manual_seed(0)
        m = Siren(dim=3, hidden_size=256, n_layers=L, c_dim=0).to(dev)
        if fitted:
            opt = torch.optim.Adam(m.parameters(), lr=1e-4)
            g = torch.Generator(device="cpu").manual_seed(0)
            for _ in range(300):
                x = ((torch.rand(4096, 3, generator=g) - 0.5) * 3.0).to(dev)
                loss = ((m(x).sdf - (x.norm(dim=-1, keepdim=True) - 1.0)) ** 2).mean()
                opt.zero_grad(); loss.backward(); opt.step()
        for p in m.parameters():
            p.requires_grad_(False)
        _models[key] = m.eval()
    return _models[key]


def _lib():
    from iso_points_amd import _lib as L
    return L.load()


def _run(dev, model, pts, form, hidden=256, T=T):
    """evaluation and a T-iteration projection of pts (1, n, 3) under step form `form`"""
    from iso_points_amd.levelset_sampling import UniformProjection, full_lengths
    from iso_points_amd.sdf_models import siren_sdf_and_grad
    lib = _lib()
    n = pts.shape[1]
    L = len(model.net) - 2
    off = lib.iso_project_siren_counts_offset(n, hidden, L)
    assert lib.iso_siren_set_step_form(form) == 0
    try:
        proj = UniformProjection()
        sdf, grad = siren_sdf_and_grad(model, pts[0])
        r = proj._project_points(model, pts, full_lengths(pts), proj_max_iters=T)
        torch.cuda.synchronize()
        counts = proj._packed_cache._ws[off:off + 64 * 4].view(torch.int32)[1:T + 1].clone()
    finally:
        lib.iso_siren_set_step_form(1)
    return sdf, grad, r.points, r.normals, r.mask, counts


NAMES = ("sdf", "grad", "points", "normals", "mask", "counts")


@pytest.mark.parametrize("fitted", [True, False])
@pytest.mark.parametrize("L", [2, 3])
def test_on_chip_form_equals_the_eight_wave_form(dev, L, fitted):
    lib = _lib()
    m = _siren(dev, L, fitted)
    assert lib.iso_siren_get_gemm_mode() == 1
    lib.iso_siren_set_step_form(1)
    assert lib.iso_siren_step_form_used(256, L, 0) == 1
    for n in SIZES:
        pts = (sphere_cloud(n, seed=n) * 0.9).to(dev)
        a, b = _run(dev, m, pts, 1), _run(dev, m, pts, 0)
        for x, y, nm in zip(a, b, NAMES):
            assert torch.equal(x, y), (n, nm, int((x != y).sum()))
        assert int(a[5][0]) <= n and (n < 100 or int(a[5][0]) > 0)          # (the counters, not some other words)


def test_coded_network_keeps_its_kernels_and_its_results(dev):
    """two codes, n = 197: a latent-coded SIREN runs the eight-wave kernels under either setting"""
    from iso_points_amd.sdf_models import CodeRows, Siren, siren_sdf_and_grad
    lib = _lib()
    torch.manual_seed(1)
    m = Siren(dim=3, hidden_size=256, n_layers=3, c_dim=8).to(dev)
    for p in m.parameters():
        p.requires_grad_(False)
    n = 197
    pts = (sphere_cloud(n, seed=5)[0] * 0.9).to(dev).contiguous()
    codes = torch.randn(2, 8, generator=torch.Generator().manual_seed(2)).to(dev)
    code_of = (torch.arange(n) >= 100).to(torch.int32).to(dev)
    outs = []
    for form in (1, 0):
        assert lib.iso_siren_set_step_form(form) == 0
        try:
            assert lib.iso_siren_step_form_used(256, 3, 1) == 0
            outs.append(siren_sdf_and_grad(m, pts, code=CodeRows(codes, code_of)))
            torch.cuda.synchronize()
        finally:
            lib.iso_siren_set_step_form(1)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_routing(dev):
    """The setter reads back; the on-chip kernels serve hidden size 256 with two or three hidden layers in the split-fp16
    mode and nothing else; the shapes they do not serve, and forward-only evaluation, give the same under either setting."""
    from iso_points_amd.sdf_models import Siren, siren_sdf_and_grad
    lib = _lib()
    try:
        assert lib.iso_siren_set_step_form(0) == 0 and lib.iso_siren_get_step_form() == 0
        assert all(lib.iso_siren_step_form_used(256, L, 0) == 0 for L in range(0, 9))
        assert lib.iso_siren_set_step_form(2) != 0 and lib.iso_siren_get_step_form() == 0
        assert lib.iso_siren_set_step_form(1) == 0 and lib.iso_siren_get_step_form() == 1
        assert [lib.iso_siren_step_form_used(256, L, 0) for L in range(0, 6)] == [0, 0, 1, 1, 0, 0]
        assert [lib.iso_siren_step_form_used(H, 3, 0) for H in (64, 128, 512)] == [0, 0, 0]
        assert lib.iso_siren_step_form_used(256, 3, 1) == 0
        lib.iso_siren_set_gemm_mode(0)
        assert lib.iso_siren_step_form_used(256, 3, 0) == 0
        lib.iso_siren_set_gemm_mode(1)
        # the launch count of a projection does not depend on the form
        for form in (0, 1):
            lib.iso_siren_set_step_form(form)
            assert lib.iso_siren_step_launches(256, 3, 10) == 5 and lib.iso_siren_step_launches(256, 3, 3) == 3
    finally:
        lib.iso_siren_set_gemm_mode(1)
        lib.iso_siren_set_step_form(1)
    n = 24609
    pts = (sphere_cloud(n, seed=7) * 0.9).to(dev)
    for H, L in ((256, 1), (256, 4), (128, 3)):
        torch.manual_seed(H + L)
        m = Siren(dim=3, hidden_size=H, n_layers=L, c_dim=0).to(dev)
        for p in m.parameters():
            p.requires_grad_(False)
        a, b = _run(dev, m, pts, 1, hidden=H, T=3), _run(dev, m, pts, 0, hidden=H, T=3)
        for x, y, nm in zip(a, b, NAMES):
            assert torch.equal(x, y), (H, L, nm)
    m = _siren(dev, 3, False)
    outs = []
    for form in (1, 0):
        lib.iso_siren_set_step_form(form)
        try:
            outs.append(siren_sdf_and_grad(m, pts[0], need_grad=False)[0])
            torch.cuda.synchronize()
        finally:
            lib.iso_siren_set_step_form(1)
    assert torch.equal(outs[0], outs[1])


def test_on_chip_form_repeats(dev):
    """the 60 000-point projection under form 1, twice in one process: identical"""
    m = _siren(dev, 3, False)
    pts = (sphere_cloud(60000, seed=60000) * 0.9).to(dev)
    a, b = _run(dev, m, pts, 1), _run(dev, m, pts, 1)
    for x, y, nm in zip(a, b, NAMES):
        assert torch.equal(x, y), nm
