"""Every kernel form of iso_farthest_point_sampling (csrc/fps.hip: four kernels in eleven template instances, picked from
p_stride alone) against the CPU oracle, through the C entry itself so that start, n_samples, lengths and out_stride are
the test's own: both ends of every form's range, the edges of the C contract, the extremes of scale, and run-to-run
identity.  FORMS is also read by tests/test_fps_forms_cpu.py, which checks without a GPU that it reaches every FPS kernel
of the built library."""
import contextlib
import functools
import os
import time

import pytest
import torch

from util import FPS_F64_SLACK, fps_float64_deficit, sphere_cloud

pytestmark = pytest.mark.gpu

NO_COOP = "ISO_FPS_NO_COOPERATIVE"
ONE_WG = "ISO_FPS_ONE_WORKGROUP"
SENTINEL = -7

# (p_stride, environment switch or None, form code: 0 k_fps, 100 + PPT k_fps_reg, 200 + PPT k_fps_lazy, 300 + PPT k_fps_grid):
# one shape on each side of every boundary of the dispatch, and one inside the ranges no other test enters
FORMS = [
    (1, None, 101), (1024, None, 101),
    (1025, None, 102), (1500, None, 102), (2000, None, 102), (2048, None, 102),
    (2049, None, 104), (4095, None, 104),
    (4096, None, 201), (131072, None, 201),
    (131073, None, 202), (200000, None, 202), (262144, None, 202),
    (262145, None, 204), (524288, None, 204),
    (524289, None, 208), (1048576, None, 208),
    (1048577, None, 216), (2097152, None, 216),
    (2097153, None, 316), (4194304, None, 316),
    (4194305, None, 0),
    (4096, NO_COOP, 104), (4097, NO_COOP, 108), (5000, NO_COOP, 108), (8192, NO_COOP, 108),
    (8193, NO_COOP, 0),
    (3000, ONE_WG, 0),
]

# above this many point-sample pairs the oracle (65 ms per sample at 2 M points) gives the first 32 samples only -- the
# first m samples of a longer run ARE the m-sample run -- and k_fps the full length
ORACLE_PAIRS = 5e7


def _ids(cases):
    return ["%d%s" % (c[0], "-" + c[1][8:].lower() if c[1] else "") for c in cases]


def _O():
    from oracle import iso_oracle as O
    return O


@contextlib.contextmanager
def _switch(env):
    """The library reads its switches on every call: set for the calls inside, gone afterwards."""
    assert NO_COOP not in os.environ and ONE_WG not in os.environ
    if env:
        os.environ[env] = "1"
    try:
        yield
    finally:
        if env:
            del os.environ[env]


def _assert_form(p, env, code):
    """A refused cooperative grid must fail here, loudly, not pass through the fallback."""
    from iso_points_amd import _lib
    lib = _lib.load()
    with _switch(env):
        on_device, by_size = lib.iso_farthest_point_sampling_form(p, 1), lib.iso_farthest_point_sampling_form(p, 0)
    assert on_device == by_size == code, (p, env, on_device, by_size, code)


def _fps(pts, lengths, n_samples, start, out_stride, env=None):
    """pts (N, P, 3) f32 on the GPU -> out_idx (N, out_stride) on the CPU, pre-filled with SENTINEL."""
    from iso_points_amd import _lib
    N, P = pts.shape[0], pts.shape[1]
    assert pts.is_contiguous() and pts.dtype == torch.float32
    dev = pts.device

    def i64(v):
        return None if v is None else torch.tensor(v, dtype=torch.int64, device=dev)
    ln, ns, st = i64(lengths), i64(n_samples), i64(start)
    work = torch.empty((_lib.load().iso_farthest_point_sampling_work_floats(N, P),), dtype=torch.float32, device=dev)
    out = torch.full((N, out_stride), SENTINEL, dtype=torch.int64, device=dev)
    with _switch(env):
        _lib.call("iso_farthest_point_sampling", _lib.ptr(pts), _lib.ptr(ln), _lib.ptr(ns), _lib.ptr(st), N, P, out_stride,
                  _lib.ptr(work), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return out.cpu()


def _expected_row(cloud, n_samples, start, out_stride):
    """The contract for one cloud (its valid rows only): start clamped into [0, len), the count clamped to len, the rest
    of the row untouched; an empty cloud's row is untouched."""
    row = torch.full((out_stride,), SENTINEL, dtype=torch.int64)
    n = cloud.shape[0]
    if n > 0 and n_samples > 0:
        m = min(n_samples, n)
        row[:m] = _O().farthest_point_sampling(cloud, m, start=min(max(start, 0), n - 1))
    return row


def _n_samples(p, code):
    if code // 100 == 2:
        return 641            # > 5 kFpsMaxRun (128): at least six exchanges, both tag phases and both slot banks reused
    if code // 100 == 3:
        return 160            # k_fps_grid exchanges every sample: both banks, both tags, 40 times each
    if p > 4194304:
        return 32
    return min(p, 257)        # odd; both LDS banks of k_fps_reg many times over


# ---- (a) every form at both ends of its range, (d) twice ----------------------------------------------------------------
@pytest.mark.parametrize("p,env,code", FORMS, ids=_ids(FORMS))
def test_every_form_against_the_oracle(dev, p, env, code):
    """A full-length sphere cloud (every register slot of every thread holds a real point up to the cloud's end; the last
    point moved out to four times the radius: at least 2.9 from every other point, which are at most 2.1 apart), a start inside the cloud, index for index against the oracle; where the oracle is affordable for the whole run also the
    float64 statement of the definition (util.fps_float64_deficit).  Run twice: the same indices."""
    _assert_form(p, env, code)
    ns = _n_samples(p, code)
    cloud = sphere_cloud(p, seed=1000 + p % 997)
    cloud[0, -1] *= 4.0                                    # the cloud's last point, alone in the form's last slot at the
    g = cloud.to(dev)                                      # lower end of a range, is the second sample: that slot counts
    start = p // 3
    t0 = time.time()
    got = _fps(g, [p], [ns], [start], ns + 3, env)
    t1 = time.time()
    assert (got[0, ns:] == SENTINEL).all()
    assert got[0, 0] == start and int(got[0, :ns].min()) >= 0 and int(got[0, :ns].max()) < p
    assert ns == 1 or got[0, 1] == p - 1
    if p * ns <= ORACLE_PAIRS:
        ref = _O().farthest_point_sampling(cloud[0], ns, start=start)
        assert torch.equal(got[0, :ns], ref)
        deficit = fps_float64_deficit(cloud[0], got[0, :ns])
        print("float64 deficit %.3g" % deficit)
        assert deficit <= FPS_F64_SLACK
    else:
        ref = _O().farthest_point_sampling(cloud[0], 32, start=start)
        assert torch.equal(got[0, :32], ref)
        if ns > 32:
            full = _fps(g, [p], [ns], [start], ns + 3, ONE_WG)
            assert torch.equal(got, full)
    t2 = time.time()
    again = _fps(g, [p], [ns], [start], ns + 3, env)
    assert torch.equal(got, again)
    print("p_stride %d form %d: %d samples in %.3f s, reference %.2f s" % (p, code, ns, t1 - t0, t2 - t1))


# ---- (b) the edges of the C contract, one shape of each kernel -----------------------------------------------------------
EDGE_SHAPES = [(1500, None, 102), (5000, NO_COOP, 108), (20000, None, 201), (300000, None, 204), (3000, ONE_WG, 0),
               (2097153, None, 316)]


@functools.lru_cache(maxsize=2)
def _ragged(p):
    """(4, p, 3): lengths [p, 0, 5, 0.6 p]; rows beyond a cloud's length are NaN -- a kernel that reads them loses the
    sequence."""
    lens = [p, 0, 5, int(p * 0.6)]
    pts = torch.full((4, p, 3), float("nan"))
    for b, n in enumerate(lens):
        if n:
            pts[b, :n] = sphere_cloud(n, seed=50 + b)[0]
    return pts, lens


@pytest.mark.parametrize("p,env,code", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_contract_edges_ragged_batch(dev, p, env, code):
    """One call, four clouds, each with its own n_samples and start: start = -5 runs from 0; an empty cloud leaves its row
    untouched; a 5-point cloud in a p_stride-wide row (len << p_stride: all but one workgroup of the grid-wide forms hold no
    point) with n_samples = len + 7 clamps to 5 samples and start = len + 10 to len - 1, the row beyond keeps the sentinel;
    start = len + 10 on a 0.6 p_stride cloud; out_stride larger than every n_samples."""
    _assert_form(p, env, code)
    pts, lens = _ragged(p)
    big = p > 50000                                        # the oracle costs p per sample
    ns = [24 if big else 70, 10, 5 + 7, 12 if big else 45]
    start = [-5, 3, 5 + 10, lens[3] + 10]
    stride = 100
    got = _fps(pts.to(dev), lens, ns, start, stride, env)
    for b in range(4):
        assert torch.equal(got[b], _expected_row(pts[b, :lens[b]], ns[b], start[b], stride)), (b, got[b][:16])
    assert got[0, 0] == 0 and got[2, 0] == 4 and got[3, 0] == lens[3] - 1
    assert (got[1] == SENTINEL).all() and (got[2, 5:] == SENTINEL).all() and sorted(got[2, :5].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("p,env,code", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_contract_edges_null_lengths(dev, p, env, code):
    """lengths = NULL means p_stride for every cloud; n_samples = 1 writes the start alone."""
    _assert_form(p, env, code)
    cloud = _ragged(p)[0][0]
    pts = torch.stack([cloud, cloud])
    ns, start, stride = [1, 17 if p > 50000 else 33], [7, 11], 40
    got = _fps(pts.to(dev), None, ns, start, stride, env)
    for b in range(2):
        assert torch.equal(got[b], _expected_row(cloud, ns[b], start[b], stride)), (b, got[b][:16])
    assert got[0].tolist() == [7] + [SENTINEL] * (stride - 1)


@pytest.mark.parametrize("p,env,code", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_contract_edges_degenerate_clouds(dev, p, env, code):
    """Distances that tie or vanish, in p_stride-wide rows: a lattice taken whole (n_samples = len: massive ties, the
    sequence is a permutation; 14^3 points where the row holds them, 11^3 in the 1 500-wide row of k_fps_reg<2>), 600
    identical points (index 0 repeats after the start), and 250 points each present twice, sampled to 400 -- 150 samples
    past exhaustion, where every min-distance is 0.

    Why the two cooperative kernels cannot spin here (argued from csrc/fps.hip, not tried): k_fps_grid decides exactly one
    sample per exchange whatever the keys are, and a workgroup's slot always receives that exchange's tag.  k_fps_lazy ends a
    round only through s_m = mm, and mm >= 1 in every round: in the first pass of the replay each workgroup's listed keys
    are as published, in descending order, so its best listed key bl = ek[0] >= eb = ek[T - 1] and no workgroup is
    uncertain, blk = 0; the largest listed key c is not 0, because a present key is never 0 -- its low word is ~index with
    index < 2^31, whose low 31 bits are not all zero, and a cloud with len > 0 lists at least one point; then bd = 0 <= cd,
    and where cd = 0 (every distance 0: exhaustion, identical points) the test is c > 0, which holds.  lim >= 1 because the
    loop is entered with done < ns.  So the first pass always writes one sample."""
    _assert_form(p, env, code)
    side = 14 if p >= 14 ** 3 else 11
    lat = torch.stack(torch.meshgrid(*([torch.arange(float(side))] * 3), indexing="ij"), -1).view(-1, 3) * 0.1
    same = torch.full((600, 3), 0.37)
    half = sphere_cloud(250, seed=71)[0]
    dup = torch.cat([half, half])
    clouds = [lat, same, dup]
    lens = [c.shape[0] for c in clouds]
    pts = torch.full((3, p, 3), float("nan"))
    for b, c in enumerate(clouds):
        pts[b, :lens[b]] = c
    ns, start, stride = [lens[0], 50, 400], [0, 17, 3], lens[0] + 1
    got = _fps(pts.to(dev), lens, ns, start, stride, env)
    for b in range(3):
        assert torch.equal(got[b], _expected_row(clouds[b], ns[b], start[b], stride)), (b, got[b][:16])
    assert sorted(got[0, :lens[0]].tolist()) == list(range(lens[0]))
    assert got[1, :50].tolist() == [17] + [0] * 49
    assert len(set(got[2, :250].tolist())) == 250 and (got[2, 250:400] == got[2, 250]).all()


# ---- (c) the extremes of scale ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scaled_1e-18", "offset_100"])
def test_scale_extremes_all_forms_equal(dev, kind):
    """3 000 sphere points scaled by 1e-18 (squared distances of 1e-36 and below: the min-distances of the
    later samples and many of the squared coordinate differences are f32 denormals) and offset by +100 with 1e-3 extent (coordinates on a 7.6e-6 grid: massive ties): k_fps_reg<4>,
    k_fps_lazy<1> (the same cloud in a 5 000-wide row) and k_fps give one sequence, bit for bit, and it is the oracle's --
    device code keeps f32 denormals (no flush-to-zero flag in the build), as the header's contract sentence states."""
    base = sphere_cloud(3000, seed=77)[0]
    cloud = base * 1e-18 if kind == "scaled_1e-18" else 100.0 + 1e-3 * base
    n, ns, start = 3000, 1000, 5
    ref = _O().farthest_point_sampling(cloud, ns, start=start)
    wide = torch.full((1, 5000, 3), float("nan"))
    wide[0, :n] = cloud
    runs = {}
    for name, pts, env, code in (("k_fps_reg<4>", cloud[None].contiguous(), None, 104), ("k_fps_lazy<1>", wide, None, 201),
                                 ("k_fps", cloud[None].contiguous(), ONE_WG, 0)):
        _assert_form(pts.shape[1], env, code)
        runs[name] = _fps(pts.to(dev), [n], [ns], [start], ns, env)[0]
    assert torch.equal(runs["k_fps_reg<4>"], runs["k_fps"]) and torch.equal(runs["k_fps_lazy<1>"], runs["k_fps"])
    for name, got in runs.items():
        assert torch.equal(got, ref), (name, int((got != ref).nonzero()[0]))
