"""Temporal accumulation (rtmi_reproject*, core.TemporalAccumulator) on the device.

  * The kernel bit for bit against reproject_reference.reproject (numpy, written from the header): linear, rgb8, weight, stderr and the counters,
    at 61x37 and at 203x99 (many workgroups, no multiple of 8 or 64), on analytic planes and on device-rendered frames and features of
    frame_reference's sphere scene under two cameras 2 degrees apart, every test alone and all together, absent stderr, the cap, poisoned pixels.
  * The device form equals the host form, also with the outputs aliased onto the current frame's buffers.
  * TemporalAccumulator, three steps, pinhole and thin lens: bit for bit the numpy chain fed with the device's own per-view frames and features;
    with denoise= the output is denoise_reference.denoise of that chain's output.
  * A live progressive frame, the denoiser and a one-shot render are not disturbed by reproject calls.
  * The CLI's --orbit N --accumulate writes the frames of one accumulator over the orbit.
Every comparison is an equality."""
import numpy as np
import pytest

import denoise_reference as dr
import frame_reference as fr
import reproject_reference as rr
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import vec3

pytestmark = pytest.mark.gpu

SIZES = [(61, 37), (203, 99)]
ALL = dict(sigma_d=0.05, sigma_n=0.3, sigma_a=0.2)
TERMS = {"depth": dict(sigma_d=0.05), "normal": dict(sigma_n=0.3), "albedo": dict(sigma_a=0.2), "all": ALL, "none": {}}
DENOISE = dict(iterations=2, sigma_c=2.0, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def _same(g, e):
    if g is None or e is None:
        return g is None and e is None
    return np.array_equal(g, e, equal_nan=g.dtype != np.uint8)


def _check(ctx, case, what, **kw):
    """host form against the restatement -> the device's result"""
    nx, ny, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, cw = case
    zero = dict(sigma_d=0.0, sigma_n=0.0, sigma_a=0.0, max_history=rr.INF)
    kw = dict(zero, **kw)
    got = ctx.reproject((0, cam0), (1, cam1), pl, pw, ps, pf, cl, cs, cf, cw, **kw)
    exp = rr.reproject(nx, ny, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, cw, **kw)
    for g, e, n in zip(got, exp, ("linear", "rgb8", "weight", "stderr", "counters")):
        if not _same(g, e):
            bad = (g != e) & ~(np.isnan(g.astype(np.float64)) & np.isnan(e.astype(np.float64)))
            raise AssertionError((what, n, "%d of %d values differ" % (bad.sum(), bad.size)))
    assert np.array_equal(got[1], fr.quantise(got[0]))
    return got


# ---- analytic planes ----------------------------------------------------------------------------------------------------------------------------------
def plane_case(nx, ny, seed=5):
    """two planes, the camera moved sideways and a little forward (so that fy is not a whole number either); a noisy history with random
    weights; features perturbed so that each test passes some taps and fails others"""
    rng = np.random.default_rng(seed)
    planes = [(-2.0, -100.0, 0.1), (-4.0, -100.0, 100.0)]
    _, cam0 = rr.flat_camera(nx, ny)
    _, cam1 = rr.flat_camera(nx, ny, origin=(0.3, 0.05, -0.02), kind=1)
    pf, pcol, _, _ = rr.plane_view(nx, ny, cam0, planes, rr.linear_colour)
    cf, ccol, _, _ = rr.plane_view(nx, ny, cam1, planes, rr.linear_colour)
    pf[..., 3:6] += 0.15 * rng.normal(size=(ny, nx, 3))
    pf[..., 0:3] += 0.1 * rng.normal(size=(ny, nx, 3))
    pf[..., 6] *= 1.0 + 0.03 * rng.normal(size=(ny, nx))
    pl = pcol + 0.05 * rng.normal(size=(ny, nx, 3))
    cl = ccol + 0.2 * rng.normal(size=(ny, nx, 3))
    pw = rng.integers(1, 60, (ny, nx)).astype(np.float64)
    ps, cs = 0.05 * rng.random((ny, nx)), 0.2 * rng.random((ny, nx))
    return [nx, ny, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, 4.0]


def poison(case, seed=9):
    """every kind of bad value, scattered: in the history (colour, weight, stderr, coverage) and in the current frame (colour, stderr, coverage, depth)"""
    nx, ny, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, cw = [a.copy() if isinstance(a, np.ndarray) else a for a in case]
    rng = np.random.default_rng(seed)
    pick = lambda n=12: (rng.integers(0, ny, n), rng.integers(0, nx, n))
    for v in (np.nan, np.inf, -np.inf):
        y, x = pick()
        pl[y, x, rng.integers(0, 3, len(y))] = v
        y, x = pick()
        cl[y, x, rng.integers(0, 3, len(y))] = v
    for v in (0.0, -1.0, np.nan, np.inf, 1e-300, 1e300):
        y, x = pick()
        pw[y, x] = v
    for v in (np.nan, np.inf):
        y, x = pick()
        ps[y, x] = v
        y, x = pick()
        cs[y, x] = v
    for v in (0.5, 0.0, np.nan, 1.0000000000000002):
        y, x = pick()
        pf[y, x, 7] = v
        y, x = pick()
        cf[y, x, 7] = v
    for v in (0.0, -1.0, np.nan, np.inf, 1e300):
        y, x = pick(6)
        cf[y, x, 6] = v
        y, x = pick(6)
        pf[y, x, 6] = v
    return [nx, ny, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, cw]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement_on_planes(ctx, size):
    case = plane_case(*size)
    n = size[0] * size[1]
    shares = {}
    for name, sig in TERMS.items():
        got = _check(ctx, case, name, **sig)
        shares[name] = int(got[4][1]) / n
        assert int(got[4][0]) == n
    print("share of pixels with history:", {k: round(v, 3) for k, v in shares.items()})
    assert shares["all"] < min(shares["depth"], shares["normal"], shares["albedo"]) and max(shares.values()) == shares["none"] < 1.0
    assert shares["all"] > 0.05, "every test passes some taps and fails others"
    capped = _check(ctx, case, "cap", max_history=5.0, **ALL)
    assert capped[2].max() == 9.0 and (case[5] > 5).any()
    # absent stderr planes: either, both
    for which in ((6,), (9,), (6, 9)):
        c = list(case)
        for k in which:
            c[k] = None
        assert _check(ctx, c, "absent stderr %r" % (which,), **ALL)[3] is None
    # poisoned pixels, with and without the tests, capped and not
    bad = poison(case)
    _check(ctx, bad, "poisoned, all", **ALL)
    _check(ctx, bad, "poisoned, none")
    _check(ctx, bad, "poisoned, capped", max_history=3.0, sigma_d=0.05)
    # a one-sample current frame: stderr +inf everywhere
    one = list(case)
    one[9], one[11] = np.full_like(case[9], np.inf), 1.0
    got = _check(ctx, one, "one sample", **ALL)
    assert np.isinf(got[3]).all()
    # the identity camera and a camera that looks the other way
    same = list(case)
    same[3], same[8], same[10] = case[2], case[4], case[7]
    assert int(_check(ctx, same, "identity", sigma_d=0.05)[4][1]) > 0
    back = list(case)
    back[2] = case[2].copy()
    back[2][3:6] = (1.0, case[2][4], 1.0)
    back[2][6:9] = (-2.0, 0.0, 0.0)
    assert int(_check(ctx, back, "turned away")[4][1]) == 0


# ---- device-rendered frames and features --------------------------------------------------------------------------------------------------------------
def _turned(nx, ny, degrees, lens=False):
    a = np.radians(degrees)
    return fr._camera(nx, ny, vec3(7.0 * np.sin(a), 8.0, 7.0 * np.cos(a)), vec3(0, 0, 0), 35, lens)


def _view(ds, camera, nx, ny, ns, na, seed):
    """the device's own frame of one view -> (cam24, linear, stderr, features)"""
    ds.set_camera(camera)
    lin, _, se, _ = ds.render_progressive(nx, ny, 0, ns, fr.DEPTH, seed)
    ft, _ = ds.render_features(nx, ny, na, seed)
    return fl.flatten_camera(camera)[1], lin, se, ft


@pytest.fixture(scope="module")
def sphere_views(ctx):
    out = {}
    for nx, ny in SIZES:
        ds = core.DeviceScene(fr.scene("spheres", nx, ny), ctx=ctx)
        try:
            out[nx, ny] = [_view(ds, _turned(nx, ny, 2.0 * k), nx, ny, 4, 3, fr.SEED + k) for k in range(2)]
        finally:
            ctx.progressive_release()
            ds.close()
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement_on_rendered_views(ctx, sphere_views, size):
    nx, ny = size
    (cam0, l0, s0, f0), (cam1, l1, s1, f1) = sphere_views[size]
    assert not np.array_equal(cam0, cam1) and 0.3 < (f1[..., 7] == 1.0).mean()
    case = [nx, ny, cam0, cam1, l0, np.full((ny, nx), 4.0), s0, f0, l1, s1, f1, 4.0]
    shares = {}
    for name, sig in TERMS.items():
        shares[name] = int(_check(ctx, case, name, **sig)[4][1]) / (nx * ny)
    print("sphere scene, 2 degrees: share of pixels with history:", {k: round(v, 3) for k, v in shares.items()})
    assert 0.2 < shares["all"] <= shares["depth"] <= shares["none"]
    _check(ctx, case, "library defaults", max_history=core.REPROJECT_MAX_HISTORY, sigma_d=core.REPROJECT_SIGMA_D, sigma_n=core.REPROJECT_SIGMA_N,
           sigma_a=core.REPROJECT_SIGMA_A)
    _check(ctx, poison(case), "poisoned", max_history=6.0, **ALL)


# ---- host form, device form, aliasing -----------------------------------------------------------------------------------------------------------------
def test_device_form_equals_host_form_and_outputs_may_alias_the_current_frame(ctx):
    torch = pytest.importorskip("torch")
    nx, ny = SIZES[0]
    case = poison(plane_case(nx, ny))
    _, _, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, cw = case
    host = ctx.reproject((0, cam0), (0, cam1), pl, pw, ps, pf, cl, cs, cf, cw, max_history=20.0, **ALL)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [dev(a) for a in (pl, pw, ps, pf, cl, cs, cf)]
    out = [torch.full((ny, nx, 3), -1.0, dtype=torch.float64, device="cuda"), torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda"),
           torch.full((ny, nx), -1.0, dtype=torch.float64, device="cuda"), torch.full((ny, nx), -1.0, dtype=torch.float64, device="cuda"),
           torch.full((2,), 77, dtype=torch.int64, device="cuda")]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.reproject_device(nx, ny, (0, cam0), (0, cam1), *d, cw, *out, max_history=20.0, stream=st.cuda_stream, **ALL)
    st.synchronize()
    for g, e, n in zip(out, host, ("linear", "rgb8", "weight", "stderr", "counters")):
        assert _same(g.cpu().numpy().astype(e.dtype), e), n
    # outputs aliased onto the current frame's buffers, on the context's own stream, no counters and no 8-bit frame
    ctx.reproject_device(nx, ny, (0, cam0), (0, cam1), *d, cw, d[4], None, out[2], d[5], None, max_history=20.0, **ALL)
    ctx.denoise(cl, None, None, iterations=0)  # a host call on the same context synchronises that stream
    assert _same(d[4].cpu().numpy(), host[0]) and _same(d[5].cpu().numpy(), host[3]) and _same(out[2].cpu().numpy(), host[2])
    # the history was only read
    for t, a in zip(d[:4], (pl, pw, ps, pf)):
        assert _same(t.cpu().numpy(), a)


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "thin-lens"])
def test_accumulator_equals_the_numpy_chain(ctx, lens):
    pytest.importorskip("torch")
    nx, ny = SIZES[0]
    ns, na, seed = 4, 2, fr.SEED + 40
    cams = [_turned(nx, ny, 1.5 * k, lens) for k in range(3)]
    ds = core.DeviceScene(fr.scene("spheres-lens" if lens else "spheres", nx, ny), ctx=ctx)
    try:
        views = [_view(ds, c, nx, ny, ns, na, seed + k) for k, c in enumerate(cams)]
        chain = rr.accumulate(views, ns, 10.0, **ALL)
        filtered = [dr.denoise(c[0], c[3], v[3], **DENOISE) for c, v in zip(chain, views)]
        for denoise in (None, DENOISE):
            acc = core.TemporalAccumulator(ds, nx, ny, ns, na=na, max_history=10.0, denoise=denoise, seed=seed, **ALL)
            for k, c in enumerate(cams):
                lin, q, se, w, share = acc.step(c)
                got = [t.cpu().numpy() for t in acc.accumulated]
                want = chain[k]
                for g, e, n in zip(got, (want[0], want[1], want[3], want[2]), ("linear", "rgb8", "stderr", "weight")):
                    assert _same(g, e), (lens, denoise is not None, k, n, int((g != e).sum()))
                assert share == want[4] and (k == 0) == (share == 0.0)
                assert np.array_equal(acc.raw_rgb8.cpu().numpy(), fr.quantise(views[k][1]))
                if denoise is None:
                    assert _same(lin.cpu().numpy(), want[0]) and _same(q.cpu().numpy(), want[1]) and _same(se.cpu().numpy(), want[3])
                else:
                    for g, e, n in zip((lin, q, se), filtered[k], ("linear", "rgb8", "stderr")):
                        assert _same(g.cpu().numpy(), e), ("filtered", lens, k, n)
                assert _same(w.cpu().numpy(), want[2])
            print("%s: share of pixels with history per step %s, largest weight %.2f" % ("thin lens" if lens else "pinhole",
                                                                                         [round(c[4], 3) for c in chain], chain[-1][2].max()))
            assert chain[-1][4] > 0.2 and chain[-1][2].max() > 2 * ns
            # reset() forgets the history: the next step is a frame of its own, with the next seed
            acc.reset()
            lin, q, se, w, share = acc.step(cams[0])
            ds.set_camera(cams[0])
            own = ds.render_progressive(nx, ny, 0, ns, fr.DEPTH, seed + 3)
            assert share == 0.0 and (w.cpu().numpy() == ns).all() and _same(acc.accumulated[0].cpu().numpy(), own[0])
            # another size starts without history too
            lin, q, se, w, share = acc.step(cams[1], nx=40, ny=24)
            assert share == 0.0 and tuple(lin.shape) == (24, 40, 3)
    finally:
        ctx.progressive_release()
        ds.close()


# ---- nothing else is disturbed ------------------------------------------------------------------------------------------------------------------------
def test_reproject_disturbs_nothing():
    nx, ny = SIZES[0]
    c = core.Context(0)
    ds = core.DeviceScene(fr.scene("spheres", nx, ny), ctx=c)
    case = plane_case(nx, ny)
    _, _, cam0, cam1, pl, pw, ps, pf, cl, cs, cf, cw = case
    call = lambda: c.reproject((0, cam0), (0, cam1), pl, pw, ps, pf, cl, cs, cf, cw, **ALL)
    try:
        before = ds.render(nx, ny, 3, fr.DEPTH, fr.SEED)
        ref5 = ds.render(nx, ny, 5, fr.DEPTH, fr.SEED)
        first = call()
        ft = ds.render_features(nx, ny, 2, seed=fr.SEED)[0]
        lin, q, err, cnt = ds.render_progressive(nx, ny, 0, 3, fr.DEPTH, fr.SEED)
        assert np.array_equal(lin, before[0])
        flt = c.denoise(lin, err, ft, **DENOISE)
        again = call()
        assert all(_same(a, b) for a, b in zip(first, again))
        assert c.progressive_samples() == 3
        lin5, q5, _, cnt5 = ds.render_progressive(nx, ny, 3, 2, fr.DEPTH, fr.SEED)  # the live frame goes on as if nothing had happened
        assert np.array_equal(lin5, ref5[0]) and np.array_equal(q5, ref5[1]) and np.array_equal(cnt5, ref5[2])
        assert all(_same(a, b) for a, b in zip(c.denoise(lin, err, ft, **DENOISE), flt))
        after = ds.render(nx, ny, 3, fr.DEPTH, fr.SEED)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    finally:
        c.progressive_release()
        ds.close()
        c.close()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_orbit_accumulate(tmp_path, capsys):
    """--orbit N --accumulate: the files are the frames of one TemporalAccumulator over the orbit's cameras"""
    pytest.importorskip("torch")
    import raytrace_clj_amd as r
    from raytrace_clj_amd import camera as cam
    nx, ny, ns, views = 48, 24, 2, 3
    out = tmp_path / "o.npy"
    assert core.main([str(out), str(nx), str(ny), str(ns), "--orbit", str(views), "--accumulate", "6", "--denoise", "1"]) == 0
    text = capsys.readouterr().out
    assert len([l for l in text.splitlines() if l.startswith("history on")]) == views and "total-rays" in text
    name = lambda k, tag: tmp_path / ("o_%03d%s.npy" % (k, tag))
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(name(k, t).name for k in range(views) for t in ("", ".acc", ".acc.denoised"))
    sc = r.scene.make_random_scene(nx, ny, 11, True)
    ds = core.DeviceScene(sc)
    try:
        acc = core.TemporalAccumulator(ds, nx, ny, ns, max_history=6.0, denoise={"iterations": 1})
        shares = []
        for k, camera in enumerate(cam.orbit(sc["camera"], views, sc.get("lookat"))):
            lin, q, se, w, share = acc.step(camera)
            shares.append(share)
            assert np.array_equal(np.load(name(k, "")), acc.raw_rgb8.cpu().numpy()), k
            assert np.array_equal(np.load(name(k, ".acc")), acc.accumulated[1].cpu().numpy()), k
            assert np.array_equal(np.load(name(k, ".acc.denoised")), q.cpu().numpy()), k
        assert np.array_equal(np.load(name(0, "")), np.load(name(0, ".acc"))) and shares[0] == 0.0
        print("orbit of %d views (120 degrees apart): share of pixels with history %s" % (views, [round(s, 3) for s in shares]))
    finally:
        ds.ctx.progressive_release()
        ds.close()
