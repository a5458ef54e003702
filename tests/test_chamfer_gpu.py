"""iso_points_amd.loss.chamfer_distance / nearest_points on the GPU against brute force written here:

  * float64: torch.cdist(x.double(), y.double()) ** 2, argmin, pytorch3d's reductions, torch autograd for the gradients;
  * float32 with the project's summation order, d2 = (dx*dx + dy*dy) + dz*dz, first minimum: the index parity reference.

Every case asserts the preconditions that make an every-point comparison fair (the f32 and the float64 argmin agree, no
point has its two nearest targets within 1e-5 relative) before it compares.  Bound for f32 quantities: rel_err < 1e-5
(tests/util.py: max |a - b| / max |b|), the README's parity bound."""
import pytest
import torch

from util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


def cube(P, seed, N=1):
    return torch.rand(N, P, 3, generator=torch.Generator().manual_seed(seed))


def sphere(P, seed, radius=1.0, N=1):
    g = torch.Generator().manual_seed(seed)
    return radius * torch.nn.functional.normalize(torch.randn(N, P, 3, generator=g), dim=-1)


def random_normals(shape, seed):
    """Random directions with lengths in [0.5, 2]: the 1e-6 clamp of the cosine is inactive."""
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1)
    return d * (0.5 + 1.5 * torch.rand(*shape[:-1], 1, generator=g))


def brute32(x, y):
    """(P1,3), (P2,3) f32 on the CPU -> d2 (P1,) f32 in the project's order, first argmin."""
    dx, dy, dz = (x[:, None, c] - y[None, :, c] for c in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    return d.min(dim=1).values, d.argmin(dim=1)


def brute64(x, y):
    d = torch.cdist(x.double(), y.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    return d, d.argmin(dim=1)


def assert_fair(x, y):
    """The preconditions of an every-point comparison for one direction of one cloud pair; returns the f32 brute force."""
    d32, i32 = brute32(x, y)
    d64, i64 = brute64(x, y)
    assert torch.equal(i32, i64), "f32 and float64 argmin differ: not a fair case"
    if y.shape[0] > 1:
        two = d64.topk(2, dim=1, largest=False).values
        assert ((two[:, 1] - two[:, 0]) > 1e-5 * two[:, 1]).all(), "two nearest targets within 1e-5 relative"
    return d32, i32, d64


_PAIRS = {}


def pair(name):
    """The two clouds of test 1, and their brute force both ways, computed once."""
    if name not in _PAIRS:
        x, y = (cube(3000, 7), cube(2500, 70)) if name == "cube" else (sphere(2500, 8), sphere(3000, 80, radius=1.02))
        _PAIRS[name] = (x, y, assert_fair(x[0], y[0]), assert_fair(y[0], x[0]))
    return _PAIRS[name]


def ref_chamfer(x, y, xl, yl, xn, yn, weights, batch_reduction, point_reduction):
    """pytorch3d.loss.chamfer_distance by brute force in float64 (differentiable); padding is cut off, never read."""
    N = x.shape[0]
    cd, cn = [], []
    for n in range(N):
        a, b = x[n, : int(xl[n])].double(), y[n, : int(yl[n])].double()
        d = torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        ia, ib = d.argmin(dim=1), d.argmin(dim=0)
        sx, sy = d.gather(1, ia[:, None]).sum(), d.gather(0, ib[None, :]).sum()
        if xn is not None:
            na, nb = xn[n, : int(xl[n])].double(), yn[n, : int(yl[n])].double()
            cos = torch.nn.functional.cosine_similarity
            nx, ny = (1 - cos(na, nb[ia], dim=1, eps=1e-6).abs()).sum(), (1 - cos(nb, na[ib], dim=1, eps=1e-6).abs()).sum()
        else:
            nx = ny = torch.zeros((), dtype=torch.float64)
        if point_reduction == "mean":
            sx, sy, nx, ny = sx / int(xl[n]), sy / int(yl[n]), nx / int(xl[n]), ny / int(yl[n])
        cd.append(sx + sy)
        cn.append(nx + ny)
    cd, cn = torch.stack(cd), torch.stack(cn)
    w = weights.double() if weights is not None else None
    if w is not None:
        if float(w.sum()) == 0.0:
            z = cd * 0.0
            return (z, z) if batch_reduction is None else (z.sum(), z.sum())
        cd, cn = cd * w, cn * w
    if batch_reduction is not None:
        cd, cn = cd.sum(), cn.sum()
        if batch_reduction == "mean":
            div = w.sum() if w is not None else N
            cd, cn = cd / div, cn / div
    return cd, cn


def gpu_chamfer(dev, x, y, xl, yl, xn, yn, weights, batch_reduction, point_reduction):
    from iso_points_amd.loss import chamfer_distance
    to = lambda t: t.to(dev) if t is not None else None  # noqa: E731
    return chamfer_distance(to(x), to(y), to(xl), to(yl), to(xn), to(yn), to(weights), batch_reduction, point_reduction)


# ---------------------------------------------------------------------------------------------- 1. indices and distances
@pytest.mark.parametrize("name", ["cube", "sphere"])
def test_indices_and_distances(dev, name):
    from iso_points_amd.loss import nearest_points
    x, y, fwd, bwd = pair(name)
    for a, b, (d32, i32, d64) in ((x, y, fwd), (y, x, bwd)):
        d2, idx = nearest_points(a.to(dev), b.to(dev))
        assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and d2.shape == a.shape[:2]
        assert torch.equal(idx[0].cpu(), i32)
        want = d64.min(dim=1).values
        err = ((d2[0].cpu().double() - want).abs() / want).max().item()
        print("%s %d -> %d: d2 max rel err %.3g" % (name, a.shape[1], b.shape[1], err))
        assert err < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2. ties
def test_ties_go_to_the_lower_index(dev):
    from iso_points_amd.loss import nearest_points
    x, y, (d32, i32, _), _ = pair("cube")
    y2 = torch.cat([y, y[:, :50]], dim=1)                       # rows 2500..2549 are exact copies of rows 0..49
    d2, idx = nearest_points(x.to(dev), y2.to(dev))
    hit = i32 < 50
    assert hit.any(), "no query has a duplicated nearest point"
    assert torch.equal(idx[0].cpu(), i32)                       # every query, the duplicated ones included: the lower index
    # and with the copies FIRST, the copies win
    y3 = torch.cat([y[:, :50], y], dim=1)
    _, idx3 = nearest_points(x.to(dev), y3.to(dev))
    assert torch.equal(idx3[0].cpu(), torch.where(hit, i32, i32 + 50))


# -------------------------------------------------------------------------------------------------------------- 3. values
def ragged_batch():
    x, y = cube(700, 21, N=2), cube(650, 22, N=2)
    xn, yn = random_normals((2, 700, 3), 23), random_normals((2, 650, 3), 24)
    xl, yl = torch.tensor([700, 300]), torch.tensor([300, 650])
    for t, l in ((x, xl), (y, yl), (xn, xl), (yn, yl)):
        for n in range(2):
            t[n, int(l[n]):] = float("nan")                    # padding that must never be read
    return x, y, xl, yl, xn, yn


def check_values(dev, x, y, xl, yl, xn, yn, weights, what):
    for n in range(x.shape[0]):
        assert_fair(x[n, : int(xl[n])], y[n, : int(yl[n])])
        assert_fair(y[n, : int(yl[n])], x[n, : int(xl[n])])
    for pr in ("mean", "sum"):
        for br in ("mean", "sum", None):
            want_d, want_n = ref_chamfer(x, y, xl, yl, xn, yn, weights, br, pr)
            got_d, got_n = gpu_chamfer(dev, x, y, xl, yl, xn, yn, weights, br, pr)
            assert got_d.shape == want_d.shape
            e = rel_err(got_d, want_d)
            print("%s %s/%s: cham_dist rel err %.3g" % (what, pr, br, e))
            assert e < TOL
            if xn is None:
                assert got_n is None
            else:
                e = rel_err(got_n, want_n)
                print("%s %s/%s: cham_normals rel err %.3g" % (what, pr, br, e))
                assert e < TOL


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_values_ragged_batch(dev, weighted, normals):
    x, y, xl, yl, xn, yn = ragged_batch()
    w = torch.tensor([0.3, 1.7]) if weighted else None
    check_values(dev, x, y, xl, yl, xn if normals else None, yn if normals else None, w, "ragged")


def test_values_full_clouds_without_lengths(dev):
    from iso_points_amd.loss import chamfer_distance
    x, y, _, _ = pair("sphere")
    xn, yn = random_normals((1, 2500, 3), 25), random_normals((1, 3000, 3), 26)
    full = lambda t: torch.tensor([t.shape[1]])  # noqa: E731
    want_d, want_n = ref_chamfer(x, y, full(x), full(y), xn, yn, None, "mean", "mean")
    got_d, got_n = chamfer_distance(x.to(dev), y.to(dev), x_normals=xn.to(dev), y_normals=yn.to(dev))
    assert rel_err(got_d, want_d) < TOL and rel_err(got_n, want_n) < TOL


@pytest.mark.parametrize("p1,p2", [(1, 400), (400, 1), (1, 1)])
def test_values_single_point_clouds(dev, p1, p2):
    x, y = cube(p1, 31), cube(p2, 32)
    xn, yn = random_normals((1, p1, 3), 33), random_normals((1, p2, 3), 34)
    check_values(dev, x, y, torch.tensor([p1]), torch.tensor([p2]), xn, yn, None, "%dx%d" % (p1, p2))


def test_values_one_weight_zero_and_all_weights_zero(dev):
    x, y = cube(300, 41, N=3), cube(260, 42, N=3)
    xn, yn = random_normals((3, 300, 3), 43), random_normals((3, 260, 3), 44)
    xl, yl = torch.tensor([300, 200, 300]), torch.tensor([260, 260, 100])
    check_values(dev, x, y, xl, yl, xn, yn, torch.tensor([0.5, 0.0, 2.0]), "one weight zero")
    for br, shape in (("mean", ()), ("sum", ()), (None, (3,))):
        xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        from iso_points_amd.loss import chamfer_distance
        d, nn = chamfer_distance(xg, yg, xl.to(dev), yl.to(dev), xn.to(dev), yn.to(dev), torch.zeros(3, device=dev), br, "mean")
        assert tuple(d.shape) == shape and tuple(nn.shape) == shape
        assert (d == 0).all() and (nn == 0).all()
        (d.sum() + nn.sum()).backward()
        assert (xg.grad == 0).all() and (yg.grad == 0).all()


def test_zero_normal_is_finite_and_follows_the_formula(dev):
    x, y = cube(300, 51), cube(260, 52)
    xn, yn = random_normals((1, 300, 3), 53), random_normals((1, 260, 3), 54)
    xn[0, 7] = 0.0
    yn[0, 11] = 0.0
    want_d, want_n = ref_chamfer(x, y, torch.tensor([300]), torch.tensor([260]), xn, yn, None, "sum", "sum")
    got_d, got_n = gpu_chamfer(dev, x, y, None, None, xn, yn, None, "sum", "sum")
    assert torch.isfinite(got_n).all() and rel_err(got_n, want_n) < TOL and rel_err(got_d, want_d) < TOL
    # the zero normal's own term is exactly 1 - |0 / (1e-6 |b|)| = 1: the sum moves by exactly the term it replaced
    from iso_points_amd.loss import _nearest
    f = lambda t: t.to(dev).float().contiguous()  # noqa: E731
    _, _, nterm, _ = _nearest(f(x), f(y), torch.tensor([300], device=dev), torch.tensor([260], device=dev), f(xn), f(yn))
    assert nterm[0, 7].item() == 1.0


# ----------------------------------------------------------------------------------------------------------- 4. gradients
def grad_case(dev, x, y, xn, yn, xl=None, yl=None, seed=90):
    """Gradients of <v, chamfer(batch_reduction=None)> for a random upstream vector v and random weights, both terms."""
    from iso_points_amd.loss import chamfer_distance
    N = x.shape[0]
    g = torch.Generator().manual_seed(seed)
    w, v, vn = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)
    xl = torch.tensor([x.shape[1]] * N) if xl is None else xl
    yl = torch.tensor([y.shape[1]] * N) if yl is None else yl
    ref_in = [t.clone().double().requires_grad_(True) for t in (x, y, xn, yn)]
    rd, rn = ref_chamfer(ref_in[0], ref_in[1], xl, yl, ref_in[2], ref_in[3], w, None, "mean")
    ((rd * v.double()).sum() + (rn * vn.double()).sum()).backward()
    gpu_in = [t.clone().to(dev).requires_grad_(True) for t in (x, y, xn, yn)]
    gd, gn = chamfer_distance(gpu_in[0], gpu_in[1], xl.to(dev), yl.to(dev), gpu_in[2], gpu_in[3], w.to(dev), None, "mean")
    ((gd * v.to(dev)).sum() + (gn * vn.to(dev)).sum()).backward()
    out = []
    for name, a, b in zip(("x", "y", "x_normals", "y_normals"), gpu_in, ref_in):
        got, want = a.grad.cpu(), torch.nan_to_num(b.grad, nan=0.0)
        assert torch.isfinite(got).all()
        e = rel_err(got, want)
        print("grad %s: rel err %.3g" % (name, e))
        out.append(e)
    assert max(out) < TOL, out
    return gpu_in


def chosen_counts(x, y):
    """How many points of x chose each point of y (float64 brute force)."""
    return torch.bincount(brute64(x, y)[1], minlength=y.shape[0])


def test_gradients_700_vs_300(dev):
    # two density levels in x, so that some targets are chosen by many queries (more than the 8 a lane sums itself) and
    # some by none
    x = torch.cat([cube(500, 9), 0.25 * cube(200, 91)], dim=1)
    y = cube(300, 92)
    xn, yn = random_normals((1, 700, 3), 93), random_normals((1, 300, 3), 94)
    assert_fair(x[0], y[0])
    assert_fair(y[0], x[0])
    c = chosen_counts(x[0], y[0])
    assert (c == 0).any() and (c > 8).any(), (int(c.min()), int(c.max()))
    c = chosen_counts(y[0], x[0])
    assert (c == 0).any()
    grad_case(dev, x, y, xn, yn)


@pytest.mark.parametrize("p1,p2", [(3000, 40), (1500, 1)])
def test_gradients_long_lists(dev, p1, p2):
    """Lists of 9..1024 entries are sorted by a wave, longer ones (here: all 1500 queries on one target) are scanned."""
    x, y = cube(p1, 95), cube(p2, 96)
    xn, yn = random_normals((1, p1, 3), 97), random_normals((1, p2, 3), 98)
    assert_fair(x[0], y[0])
    assert_fair(y[0], x[0])
    c = chosen_counts(x[0], y[0])
    assert (c.max() > 1024) if p2 == 1 else (8 < c.max() <= 1024 and c.min() > 8)
    grad_case(dev, x, y, xn, yn)


def test_gradients_scanned_list_behind_another_cloud(dev):
    """The heavy paths with more than one cloud and P1 != P2: in cloud 1 all 1200 queries choose y[1, 0], a list beyond the
    1024 a wave sorts, so the wave scans cloud 1's own index row (row stride 1300) behind cloud 0's, whose lists are sorted
    by a wave; count and offset rows have the stride max(P1, P2) = 1300, the lists of this side 1300, of the other side 40."""
    x, y = cube(1300, 101, N=2), cube(40, 102, N=2)
    xn, yn = random_normals((2, 1300, 3), 103), random_normals((2, 40, 3), 104)
    xl, yl = torch.tensor([1300, 1200]), torch.tensor([40, 1])
    for t, l in ((x, xl), (y, yl), (xn, xl), (yn, yl)):
        t[1, int(l[1]):] = float("nan")                        # padding that must never be read
    for n in range(2):
        assert_fair(x[n, : int(xl[n])], y[n, : int(yl[n])])
        assert_fair(y[n, : int(yl[n])], x[n, : int(xl[n])])
    c0, c1 = chosen_counts(x[0], y[0]), chosen_counts(x[1, :1200], y[1, :1])
    assert 8 < c0.max() <= 1024, int(c0.max())
    assert c1.max() > 1024, int(c1.max())
    gpu_in = grad_case(dev, x, y, xn, yn, xl, yl)
    # rows beyond the lengths (NaN inputs) get a zero gradient
    assert (gpu_in[0].grad[1, 1200:] == 0).all() and (gpu_in[1].grad[1, 1:] == 0).all()
    assert (gpu_in[2].grad[1, 1200:] == 0).all() and (gpu_in[3].grad[1, 1:] == 0).all()


def test_gradients_ragged_batch(dev):
    x, y, xl, yl, xn, yn = ragged_batch()
    gpu_in = grad_case(dev, x, y, xn, yn, xl, yl)
    # padded rows (NaN inputs) get a zero gradient
    assert (gpu_in[0].grad[1, 300:] == 0).all() and (gpu_in[1].grad[0, 300:] == 0).all()
    assert (gpu_in[2].grad[1, 300:] == 0).all() and (gpu_in[3].grad[0, 300:] == 0).all()


# --------------------------------------------------------------------------------------------------------- 5. determinism
def test_forward_and_backward_are_bit_identical_between_runs_and_streams(dev):
    from iso_points_amd.loss import chamfer_distance
    x, y, _, _ = pair("cube")
    xn, yn = random_normals((1, 3000, 3), 61), random_normals((1, 2500, 3), 62)

    def run():
        ins = [t.clone().to(dev).requires_grad_(True) for t in (x, y, xn, yn)]
        d, n = chamfer_distance(*ins[:2], x_normals=ins[2], y_normals=ins[3])
        (d + 0.37 * n).backward()
        return [d.detach(), n.detach()] + [t.grad for t in ins]

    first, second = run(), run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------- 6. agreement with the existing search
def test_nearest_points_equals_knn_points_k1(dev):
    from iso_points_amd.loss import nearest_points
    from iso_points_amd.point_processing import knn_points
    x, y, xl, yl, _, _ = ragged_batch()
    for a, b, al, bl in ((x, y, xl, yl), (y, x, yl, xl)):
        d2, idx = nearest_points(a.to(dev), b.to(dev), al.to(dev), bl.to(dev))
        k = knn_points(a.to(dev), b.to(dev), al.to(dev), bl.to(dev), K=1)
        for n in range(2):
            L = int(al[n])
            assert torch.equal(idx[n, :L], k.idx[n, :L, 0]) and torch.equal(d2[n, :L], k.dists[n, :L, 0])
            assert (idx[n, L:] == -1).all() and (d2[n, L:] == 0).all()


@pytest.mark.parametrize("name", ["cube", "sphere", "far"])
def test_nearest_points_equals_knn_points_k1_beyond_one_cell_block(dev, name):
    """The two searches are separate kernels with the same walk: bit for bit the same on full clouds, and on queries far
    from the target cloud, which each kernel finishes on its own second path (a wave inside the launch / the tail kernel)."""
    from iso_points_amd.loss import nearest_points
    from iso_points_amd.point_processing import knn_points
    if name == "far":
        x, y = 3.0 * cube(4000, 75) - 1.0, sphere(20000, 76)
    else:
        x, y, _, _ = pair(name)
    for a, b in ((x, y), (y, x)):
        d2, idx = nearest_points(a.to(dev), b.to(dev))
        k = knn_points(a.to(dev), b.to(dev), K=1)
        assert torch.equal(idx, k.idx[..., 0]) and torch.equal(d2, k.dists[..., 0])


def test_only_the_gradients_asked_for_are_computed(dev):
    """The trainer's case: the predicted cloud needs a gradient, the ground truth does not.  What is computed is the same bits
    as in the all-four run."""
    from iso_points_amd.loss import chamfer_distance
    x, y = cube(700, 21), cube(650, 22)
    xn, yn = random_normals((1, 700, 3), 23), random_normals((1, 650, 3), 24)

    def run(req):
        ins = [t.clone().to(dev).requires_grad_(r) for t, r in zip((x, y, xn, yn), req)]
        d, n = chamfer_distance(*ins[:2], x_normals=ins[2], y_normals=ins[3])
        (d + 0.5 * n).backward()
        return [t.grad for t in ins]

    full = run((True, True, True, True))
    for req in ((True, False, False, False), (False, True, False, False), (True, False, True, False),
                (False, False, False, True), (False, True, True, False)):
        got = run(req)
        for g, f, r in zip(got, full, req):
            assert (g is None) == (not r)
            if r:
                assert torch.equal(g, f)


def test_default_lengths_read_nothing_back(dev):
    """No device-to-host read in a call without weights and without caller-built lengths: the call can be enqueued behind
    running work."""
    from iso_points_amd.loss import chamfer_distance
    x, y = cube(700, 21).to(dev).requires_grad_(True), cube(650, 22).to(dev)
    chamfer_distance(x, y)[0].backward()                       # warm: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.grad = None
        chamfer_distance(x, y)[0].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad).all()


# ------------------------------------------------------------------------------------------------------ 7. multiple cells
def test_20000_points_spot_checked(dev):
    from iso_points_amd.loss import nearest_points
    x, y = sphere(20000, 71), sphere(20000, 72, radius=1.01)
    # a few far queries: they leave the two-ring walk and are finished by their wave
    x[0, :5] = torch.tensor([[3.0, 0.1, 0.2], [-2.5, 2.5, 0.3], [0.3, 0.2, 0.1], [0.0, -4.0, 0.0], [30.0, 30.0, -30.0]])
    d2, idx = nearest_points(x.to(dev), y.to(dev))
    pick = torch.cat([torch.arange(5), torch.randperm(20000, generator=torch.Generator().manual_seed(73))[:507]])
    # against the f32 brute force alone: the far queries see many targets at nearly the same distance, and the same
    # expression in the same precision decides them the same way
    _, i32 = brute32(x[0, pick], y[0])
    assert torch.equal(idx[0].cpu()[pick], i32)
    want = brute64(x[0, pick], y[0])[0].min(dim=1).values
    assert ((d2[0].cpu()[pick].double() - want).abs() / want).max().item() < 1e-6
