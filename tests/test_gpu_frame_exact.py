"""The back half of a frame on the device, bit for bit: reduce_kernel, assemble_kernel, assemble_region_kernel, frame_fold_kernel and
frame_resolve_kernel against references that are not the device.

  * Scenes whose colours never touch libm (frame_reference.py) must equal oracle.render EXACTLY -- linear, rgb8, both counters -- through every
    path that folds or assembles: tree and flat scan, one sample pass and many, an unaligned region, tiles dealt over 1..8 ranks and assembled,
    a progressive frame after every uneven chunk.
  * For the pinhole scenes the linear frame also equals an in-order numpy sum of the oracle's single samples, times 1 / ns
    (test_frame_reference.py shows that a reversed, pairwise, divided or restarted fold of those samples is a different frame in 40 % of the
    pixels or more), and the progressive noise plane agrees with a two-pass standard error of those samples.
  * The quantiser and the tile dealing are driven with chosen values through rtmi_assemble_device: every bucket border with its neighbours,
    the edges of the domain, NaN, tiles that encode where they belong; the two other copies of the quantiser get border values through a world
    that is one constant light.

RTMI_F32 frames: linear and the counters against the f32 oracle; rgb8 against the float64 quantiser of the device's own linear, because the device
quantises the widened mean in double for both precisions while the f32 oracle quantises in float.

Every number below is an equality, except the bound of _check_stderr, derived there."""
import ctypes as C

import numpy as np
import pytest

import frame_reference as fr
import raytrace_clj_amd as r
from raytrace_clj_amd import core

pytestmark = pytest.mark.gpu

RTMI_E_ARG = -1
REGIONS = [(5, 3, 50, 30), (13, 0, 61, 21), (8, 8, 9, 9)]
CHUNKS = (1, 1, 3, 2, 6)  # k = 1, 2, 5, 7, 13


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


def _passes(ctx):
    v = C.c_int32()
    core.check(r._ffi.lib().rtmi_last_passes(ctx.handle, C.byref(v)))
    return v.value


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_ctx():
    """a context whose sample buffer is at the floor of 1 MiB: the frames of SIZE_PASSES take >= 3 sample passes at ns = 13"""
    c = core.Context(0)
    c.set_option("workspace_bytes", 1 << 20)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_scene():
    made = {}

    def get(ctx, name, nx, ny):
        key = (id(ctx), name, nx, ny)
        if key not in made:
            made[key] = core.DeviceScene(fr.scene(name, nx, ny), ctx=ctx)
        return made[key]

    yield get
    for ds in made.values():
        ds.close()


_expected = {}


def _expect(o, name, nx, ny, ns, region=None):
    key = (o.precision, name, nx, ny, ns, region)
    if key not in _expected:
        _expected[key] = o.render(fr.scene(name, nx, ny), nx, ny, ns, fr.DEPTH, fr.SEED, region=region, nthreads=16)
    return _expected[key]


def _check(got, exp, precision, what):
    lin, q, cnt = got
    elin, eq, ecnt = exp
    assert np.array_equal(lin, elin), (what, "linear: %d of %d pixels differ" % ((lin != elin).any(axis=2).sum(), lin.shape[0] * lin.shape[1]))
    assert np.array_equal(np.asarray(cnt, np.uint64), ecnt), (what, cnt, ecnt)
    assert np.array_equal(q, fr.quantise(lin)), (what, "rgb8 against the float64 quantiser of the device's linear")
    if precision == "f64":
        assert np.array_equal(q, eq), (what, "rgb8")


def _check_fold(o, name, nx, ny, ns, lin, what, region=None):
    """the device's linear against the numpy in-order fold of the oracle's samples (pinhole scenes)"""
    if name == "spheres-lens":
        return
    smp, _ = fr.samples(o, name, nx, ny, ns)
    ref = fr.frame_in_order(smp)
    if region is not None:
        x0, y0, x1, y1 = region
        ref = ref[y0:y1, x0:x1]
    assert np.array_equal(lin, ref), (what, "against the numpy fold")


def _check_stderr(err, smp, k, what, region=None):
    """frame_resolve_kernel's noise plane against the two-pass reference.

    The bound.  The device keeps Welford's M2 in double, the reference is two-pass; with S the exact sum of squared deviations of a channel's k
    samples, M the largest |sample| of the pixel, u = eps / 2:
      Welford (West's updating form; Chan, Golub & LeVeque 1983):  |dS| <= k u kappa S with kappa = sqrt(sum x^2 / S), i.e. |dS| <= k u sqrt(k) M sqrt(S);
      se = sqrt(S / (k (k - 1))) and |sqrt(S + dS) - sqrt(S)| <= |dS| / sqrt(S), so |d se| <= k u sqrt(k) M / sqrt(k (k - 1)) <= k u M  (k >= 2);
      two-pass:  |dS| <= k u S + k^2 u^2 sum x^2, which moves se by at most (k u / 2) se + k u M <= 1.5 k u M  (se <= M);
      the divisions and the root of either side: 3 u se each.
    Together under (2.5 k + 6) u M <= 2 k eps M for k >= 2; the analyses are first order, so four times that: 8 k eps M.  Against a standard error
    of the order of M / sqrt(k) that is a relative 1e-14.  A pixel whose samples are all equal is exactly 0, k = 1 is +inf."""
    ref, big = fr.stderr_two_pass(smp, k), fr.largest_sample(smp, k)
    equal = fr.to_image((smp[:, :, :k] == smp[:, :, :1]).all(axis=2).astype(np.float64)).all(axis=2)
    if region is not None:
        x0, y0, x1, y1 = region
        ref, big, equal = ref[y0:y1, x0:x1], big[y0:y1, x0:x1], equal[y0:y1, x0:x1]
    assert err.shape == ref.shape
    if k == 1:
        assert np.isposinf(err).all(), what
        return
    assert (err[equal] == 0).all() and (err[~equal] > 0).all(), what
    unit = k * np.finfo(np.float64).eps * big
    lit = unit > 0
    print(what, "stderr: largest |device - reference| / (k eps M) = %.3g" % (np.abs(err - ref)[lit] / unit[lit]).max())
    excess = np.abs(err - ref) - 8 * unit
    assert (excess <= 0).all(), (what, float(excess.max()))


# ---- 1. libm-free scenes against the oracle, through every path that folds or assembles ---------------------------------------------------------
@pytest.mark.parametrize("name,precision", fr.CASES)
def test_one_shot_tree_and_flat_scan(request, ctx, device_scene, name, precision):
    o = _oracle(request, precision)
    nx, ny = fr.SIZE
    ds = device_scene(ctx, name, nx, ny)
    try:
        for accel in (1, 0):
            ctx.set_option("accel", accel)
            for ns in fr.NS_EDGE + fr.NS_FOLD:
                lin, q, cnt = ds.render(nx, ny, ns, precision=precision)
                assert ctx.last_accel() == ("bvh" if accel else "flat") and _passes(ctx) == 1
                _check((lin, q, cnt), _expect(o, name, nx, ny, ns), precision, (name, precision, "accel", accel, "ns", ns))
                _check_fold(o, name, nx, ny, ns, lin, (name, precision, accel, ns))
    finally:
        ctx.set_option("accel", 1)


@pytest.mark.parametrize("name,precision", fr.CASES)
def test_many_sample_passes(request, small_ctx, device_scene, name, precision):
    """accum carries the running sum over >= 2 pass boundaries, one-shot and inside a progressive call"""
    o = _oracle(request, precision)
    nx, ny = fr.SIZE_PASSES[name]
    ns = fr.NS_MAX
    ds = device_scene(small_ctx, name, nx, ny)
    exp = _expect(o, name, nx, ny, ns)
    lin, q, cnt = ds.render(nx, ny, ns, precision=precision)
    assert _passes(small_ctx) >= 3
    _check((lin, q, cnt), exp, precision, (name, precision, "one-shot"))
    _check_fold(o, name, nx, ny, ns, lin, (name, precision, "one-shot, many passes"))
    try:
        plin, pq, err, pcnt = ds.render_progressive(nx, ny, 0, 5, precision=precision)
        assert _passes(small_ctx) >= 2
        _check((plin, pq, pcnt), _expect(o, name, nx, ny, 5), precision, (name, precision, "progressive, k = 5"))
        plin, pq, err, pcnt = ds.render_progressive(nx, ny, 5, 8, precision=precision)
        assert _passes(small_ctx) >= 2
        _check((plin, pq, pcnt), exp, precision, (name, precision, "progressive, k = 13"))
        _check_fold(o, name, nx, ny, ns, plin, (name, precision, "progressive, many passes"))
        if name != "spheres-lens":
            _check_stderr(err, fr.samples(o, name, nx, ny, ns)[0], ns, (name, precision, "many passes"))
    finally:
        small_ctx.progressive_release()


@pytest.mark.parametrize("name,precision", fr.CASES)
def test_unaligned_regions(request, ctx, device_scene, name, precision):
    o = _oracle(request, precision)
    nx, ny = fr.SIZE
    ds = device_scene(ctx, name, nx, ny)
    for region, ns in zip(REGIONS, (7, 13, 7)):
        lin, q, cnt = ds.render(nx, ny, ns, precision=precision, region=region)
        _check((lin, q, cnt), _expect(o, name, nx, ny, ns, region), precision, (name, precision, region))
        _check_fold(o, name, nx, ny, ns, lin, (name, precision, region), region)


@pytest.mark.parametrize("name,precision", fr.CASES)
def test_tiles_dealt_over_ranks_and_assembled(request, ctx, device_scene, name, precision):
    import torch
    o = _oracle(request, precision)
    L = r._ffi.lib()
    nx, ny = fr.SIZE
    ds = device_scene(ctx, name, nx, ny)
    for world, ns in ((1, 7), (2, 13), (3, 7), (5, 13), (8, 7)):
        per = int(L.rtmi_local_tiles(nx, ny, 0, world))
        assert per == -(-(fr.tiles_of(nx, ny)[0] * fr.tiles_of(nx, ny)[1]) // world)
        gathered = torch.full((world, per, 64, 3), float("nan"), dtype=torch.float64, device="cuda")
        counters = torch.zeros((world, 2), dtype=torch.int64, device="cuda")
        out = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
        out8 = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for rank in range(world):
            assert int(L.rtmi_local_tiles(nx, ny, rank, world)) <= per
            ds.render_tiles_device(nx, ny, ns, rank, world, gathered[rank], counters[rank], precision=precision)
        core.check(L.rtmi_assemble_device(ctx.handle, nx, ny, world, per, r._ffi.ptr(gathered), r._ffi.ptr(out), r._ffi.ptr(out8), None))
        torch.cuda.synchronize()
        cnt = counters.cpu().numpy().sum(axis=0).astype(np.uint64)
        lin = out.cpu().numpy()
        _check((lin, out8.cpu().numpy(), cnt), _expect(o, name, nx, ny, ns), precision, (name, precision, "world", world))
        _check_fold(o, name, nx, ny, ns, lin, (name, precision, "world", world))


@pytest.mark.parametrize("name,precision", fr.CASES)
def test_progressive_after_every_uneven_chunk(request, ctx, device_scene, name, precision):
    o = _oracle(request, precision)
    nx, ny = fr.SIZE
    ds = device_scene(ctx, name, nx, ny)
    try:
        for region in (None, REGIONS[0]):
            k = 0
            for n in CHUNKS:
                lin, q, err, cnt = ds.render_progressive(nx, ny, k, n, precision=precision, region=region)
                k += n
                what = (name, precision, region, "k", k)
                _check((lin, q, cnt), _expect(o, name, nx, ny, k, region), precision, what)
                _check_fold(o, name, nx, ny, k, lin, what, region)
                if name != "spheres-lens":
                    _check_stderr(err, fr.samples(o, name, nx, ny, k)[0], k, what, region)
                else:
                    assert np.isposinf(err).all() if k == 1 else np.isfinite(err).all()
            assert k == fr.NS_MAX
    finally:
        ctx.progressive_release()


# ---- 3. the quantiser and the tile dealing on chosen inputs ------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (61, 37), (200, 100)]
WORLDS = [1, 2, 3, 5, 8]
_LIN_FILL, _Q_FILL = 123456.789, 0xAB


def _assemble(ctx, gathered, nx, ny, world, per, want_lin=True, want_q=True, null_gathered=False):
    """-> (rc, out_linear, out_rgb8) as numpy; both outputs are pre-filled, so an output that was not written shows its fill"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(gathered)).cuda()
    lin = torch.full((max(ny, 1), max(nx, 1), 3), _LIN_FILL, dtype=torch.float64, device="cuda")
    q = torch.full((max(ny, 1), max(nx, 1), 3), _Q_FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = r._ffi.lib().rtmi_assemble_device(ctx.handle, nx, ny, world, per, None if null_gathered else r._ffi.ptr(d),
                                           r._ffi.ptr(lin) if want_lin else None, r._ffi.ptr(q) if want_q else None, None)
    torch.cuda.synchronize()
    return rc, lin.cpu().numpy(), q.cpu().numpy()


def _untouched(lin, q):
    return (lin == _LIN_FILL).all() and (q == _Q_FILL).all()


def _per(nx, ny, world):
    return int(r._ffi.lib().rtmi_local_tiles(nx, ny, 0, world))


@pytest.mark.parametrize("size", SIZES)
def test_assemble_deals_every_tile_to_its_place(ctx, size):
    nx, ny = size
    for world in WORLDS:
        for extra in (0, 3):  # tiles_per_rank as needed, and larger: padding slots and out-of-frame pixels hold NaN and must not come out
            per = _per(nx, ny, world) + extra
            g, frame = fr.coded_tiles(nx, ny, world, per)
            rc, lin, q = _assemble(ctx, g, nx, ny, world, per)
            assert rc == 0 and lin.tobytes() == frame.tobytes() and np.array_equal(q, fr.quantise(frame)), (world, extra)
        rc, lin, q = _assemble(ctx, g, nx, ny, world, per, want_q=False)
        assert rc == 0 and lin.tobytes() == frame.tobytes() and (q == _Q_FILL).all(), (world, "out_rgb8 null")
        rc, lin, q = _assemble(ctx, g, nx, ny, world, per, want_lin=False)
        assert rc == 0 and (lin == _LIN_FILL).all() and np.array_equal(q, fr.quantise(frame)), (world, "out_linear null")


def test_assemble_quantises_chosen_means(ctx):
    """bucket borders and their neighbours, the edges of the domain, NaN: out_rgb8 is the reference's value, out_linear a copy of the bits"""
    vals = fr.chosen_means()
    assert len(vals) >= 255 * 5 + 20
    seen = np.zeros(len(vals), bool)
    for n, (nx, ny) in enumerate(SIZES):
        for world in WORLDS:
            shift = (7 * n + world) * 97 % len(vals)
            count = nx * ny * 3
            idx = (np.arange(count) + shift) % len(vals)
            seen[idx] = True
            frame = np.ascontiguousarray(vals[idx].reshape(ny, nx, 3))
            per = _per(nx, ny, world)
            rc, lin, q = _assemble(ctx, fr.deal(frame, world, per), nx, ny, world, per)
            assert rc == 0 and lin.tobytes() == frame.tobytes(), (nx, ny, world)  # the bytes: -0.0 and the NaNs with their signs
            bad = q != fr.quantise(frame)
            assert not bad.any(), (nx, ny, world, [(float(m).hex(), int(a), int(b)) for m, a, b in zip(frame[bad][:5], q[bad][:5], fr.quantise(frame)[bad][:5])])
    assert seen.all()


def test_assemble_quantises_random_means(ctx):
    rng = np.random.default_rng(11)
    nx, ny = 200, 100
    for world in WORLDS:  # 5 x 60 000 means in [0, 1.2)
        frame = rng.random((ny, nx, 3)) * 1.2
        per = _per(nx, ny, world)
        rc, lin, q = _assemble(ctx, fr.deal(frame, world, per), nx, ny, world, per)
        assert rc == 0 and lin.tobytes() == frame.tobytes() and np.array_equal(q, fr.quantise(frame)), world


def test_assemble_refuses_bad_arguments_and_writes_nothing(ctx):
    nx, ny, world = 61, 37, 5  # 40 tiles: 8 per rank
    per = _per(nx, ny, world)
    assert per == 8
    g, _ = fr.coded_tiles(nx, ny, world, per)
    cases = {"too few slots": dict(nx=nx, ny=ny, world=world, per=per - 1), "null gathered": dict(nx=nx, ny=ny, world=world, per=per, null_gathered=True),
             "nx = 0": dict(nx=0, ny=ny, world=world, per=per), "ny = 0": dict(nx=nx, ny=0, world=world, per=per),
             "world = 0": dict(nx=nx, ny=ny, world=0, per=per), "tiles_per_rank = 0": dict(nx=nx, ny=ny, world=world, per=0),
             "nx < 0": dict(nx=-nx, ny=ny, world=world, per=per), "world < 0": dict(nx=nx, ny=ny, world=-1, per=per)}
    for what, kw in cases.items():
        rc, lin, q = _assemble(ctx, g, kw.pop("nx"), kw.pop("ny"), kw.pop("world"), kw.pop("per"), **kw)
        assert rc == RTMI_E_ARG and r._ffi.lib().rtmi_last_error(), what
        assert _untouched(lin, q), what
    rc, lin, q = _assemble(ctx, g, nx, ny, world, per)
    assert rc == 0 and not (lin == _LIN_FILL).any()


def _light_colours(precision):
    """colours for the constant-light world, three per scene: bucket borders with their neighbours (f32: the neighbouring floats of the border),
    values above 1, +inf, a negative mean, zero"""
    R = fr.REAL[precision]
    b = fr.bucket_borders()
    vals = []
    for k in (1, 2, 128, 255):
        m = b[k - 1]
        if precision == "f64":
            vals += list(fr.around([m]))
        else:
            f = np.float32(m)
            lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
            vals += [float(x) for x in (f, lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)))]
    vals += [float(np.nextafter(R(1.0), R(0.0))), 1.0, 1.5, 15.0, 1e300, np.inf, -0.25, 0.0, 0.18, 0.5]
    assert len(vals) % 3 == 0
    return np.array(vals, np.float64).reshape(-1, 3)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_quantiser_behind_region_and_progressive_renders(request, ctx, precision):
    """assemble_region_kernel and frame_resolve_kernel have no entry of their own: a world that is one constant light of colour c has every
    sample equal to c, so the mean is (c + ... + c) * (1 / ns) in the frame's precision"""
    o = _oracle(request, precision)
    R = fr.REAL[precision]
    nx, ny, region = 19, 11, (3, 2, 17, 10)
    for c in _light_colours(precision):
        flat = fr.constant_light_scene(c)
        with np.errstate(over="ignore"):
            cr = c.astype(R)  # the colour in the frame's precision (1e300 is +inf in f32)
        ds = core.DeviceScene(flat, ctx=ctx)
        try:
            for ns in (1, 3, 7):
                acc = cr
                for _ in range(ns - 1):
                    acc = acc + cr
                mean = (acc * (R(1.0) / R(ns))).astype(np.float64)
                assert acc.dtype == R
                for rg in (region, None):
                    w, h = (rg[2] - rg[0], rg[3] - rg[1]) if rg else (nx, ny)
                    exp = (np.broadcast_to(mean, (h, w, 3)), np.broadcast_to(fr.quantise(mean), (h, w, 3)), np.array([w * h * ns, w * h], np.uint64))
                    olin, oq, ocnt = o.render(flat, nx, ny, ns, fr.DEPTH, fr.SEED, region=rg)
                    assert olin.tobytes() == np.ascontiguousarray(exp[0]).tobytes() and np.array_equal(ocnt, exp[2])  # the two references agree
                    assert precision == "f32" or np.array_equal(oq, exp[1])
                    lin, q, cnt = ds.render(nx, ny, ns, precision=precision, region=rg)
                    what = (precision, c.tolist(), ns, rg)
                    assert lin.tobytes() == olin.tobytes() and np.array_equal(q, exp[1]) and np.array_equal(cnt, exp[2]), what + ("render",)
                    k = 0
                    for n in (1, 2, 4):  # k = 1, 3, 7
                        plin, pq, err, pcnt = ds.render_progressive(nx, ny, k, n, precision=precision, region=rg)
                        k += n
                        if k == ns:
                            assert plin.tobytes() == olin.tobytes() and np.array_equal(pq, exp[1]) and np.array_equal(pcnt, exp[2]), what + ("progressive",)
                            if np.isfinite(cr).all():
                                assert np.isposinf(err).all() if k == 1 else (err == 0).all(), what
                            break
        finally:
            ctx.progressive_release()
            ds.close()
