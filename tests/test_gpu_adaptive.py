"""Adaptive sampling on the device (rtmi_render_adaptive*): 8x8 tiles stop taking samples once their noise is below eps, and what every tile
holds stays bit for bit what the one-shot render computes with as many samples.

  * libm-free scenes (frame_reference.py), cases of adaptive_reference.py: the samples behind every pixel after every round equal the schedule
    numpy derives from the oracle's individual samples; the frame equals the oracle's samples folded in order per tile, the 8-bit frame the
    float64 quantiser of it (the criterion of test_gpu_frame_exact.py); the ray counter equals the segments of exactly the samples taken.
  * scenes that use libm (cover scene, Cornell box through tree and flat scan, make-final, a region): per level n of out_samples the pixels
    equal the library's own render(ns = n); out_stderr equals a uniform progressive run's plane at k = n; the schedule equals the one
    derived from those planes.  eps is taken from the uniform run, midway inside a gap of the sorted per-tile maxima of its first round.  The
    device compares the very doubles the uniform run reports (se <= eps per channel; the plane is their maximum), so no margin is needed.
  * eps = 0, a huge eps, a tiny eps; sample passes, interleaved renders, an accel switch, a frame started by render_progressive: same bytes;
    state errors leave the frame alone; device form = host form; the CLI; one frame at 1920x1080.

Every comparison below is an equality."""
import ctypes as C
import re

import numpy as np
import pytest

import adaptive_reference as ar
import frame_reference as fr
import raytrace_clj_amd as r
from raytrace_clj_amd import core

pytestmark = pytest.mark.gpu

RTMI_E_ARG, RTMI_E_STATE = -1, -5
REGION = (37, 21, 101, 59)


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


def _passes(ctx):
    v = C.c_int32()
    core.check(r._ffi.lib().rtmi_last_passes(ctx.handle, C.byref(v)))
    return v.value


def _same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cover(ctx):
    ds = core.DeviceScene(r.scene.make_random_scene(200, 100, 11, True), ctx=ctx)
    yield ds
    ds.close()


# ---- the oracle, bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ar.CASES, ids=ar.case_id)
def test_oracle_schedule_frame_and_rays(request, ctx, case):
    name, precision, (nx, ny), first, chunk, cap, eps = case
    o = _oracle(request, precision)
    smp, nseg, rounds = ar.reference_run(o, case)
    ds = core.DeviceScene(fr.scene(name, nx, ny), ctx=ctx)
    try:
        got, lists = [], []
        for g in ds.refine_adaptive(nx, ny, cap, chunk, eps, first=first, precision=precision, depth=fr.DEPTH, seed=fr.SEED):
            got.append(g)
            lists.append(ctx.adaptive_active_tiles())  # the list the next call traces
        assert [g[0] for g in got] == [k for k, _, _, _ in rounds]
        for (k, lin, q, err, spp, cnt, active), (_, n_t, act, _), tiles in zip(got, rounds, lists):
            n_px = ar.per_pixel(n_t, nx, ny)
            assert spp.dtype == np.int32 and np.array_equal(spp, n_px), (k, "samples per pixel")
            assert active == int(act.sum()), k
            # the tiles still active, in ascending tile order
            assert tiles.dtype == np.int32 and np.array_equal(tiles, np.flatnonzero(act.ravel())), (k, "active list")
            exp = ar.expected_frame(smp, n_px)
            assert np.array_equal(lin, exp), (k, "linear: %d pixels differ" % (lin != exp).any(axis=2).sum())
            assert np.array_equal(q, fr.quantise(exp)), (k, "rgb8")
            assert int(cnt[0]) == ar.expected_rays(nseg, n_px) and int(cnt[1]) == nx * ny, (k, cnt)
        assert ctx.adaptive_status() == (int(rounds[-1][2].sum()), rounds[-1][1].size, int(ar.per_pixel(rounds[-1][1], nx, ny).sum()))
        assert ctx.progressive_samples() == cap
    finally:
        ds.close()
        ctx.progressive_release()


# ---- the library's own one-shot render, libm scenes included -----------------------------------------------------------------------------------
def _uniform(ds, nx, ny, ks, precision="f64", region=None):
    """a uniform progressive run -> {k: out_stderr plane} for the rounds ks"""
    errs, k0 = {}, 0
    for k in ks:
        _, _, err, _ = ds.render_progressive(nx, ny, k0, k - k0, precision=precision, region=region)
        errs[k], k0 = err, k
    return errs


def _full(plane, nx, ny, region):
    if region is None:
        return plane
    out = np.full((ny, nx), -np.inf)
    out[region[1]:region[3], region[0]:region[2]] = plane
    return out


def _choose_eps(errs, nx, ny, first, region=None):
    """midway inside the widest (relative) gap of the sorted per-tile maxima of the first round, looked for in the middle half"""
    v = np.unique(ar.tile_max(_full(errs[first], nx, ny, region), region))
    v = v[np.isfinite(v) & (v > 0)]
    assert len(v) >= 8, "too few distinct per-tile maxima to choose from"
    lo, hi = len(v) // 4, 3 * len(v) // 4
    i = lo + int(np.argmax(v[lo + 1:hi + 1] / v[lo:hi]))
    return float(0.5 * (v[i] + v[i + 1]))


def _crop(a, region):
    return a if region is None else a[region[1]:region[3], region[0]:region[2]]


def _check_against_uniform(ds, nx, ny, first, chunk, cap, precision="f64", region=None, eps=None, min_levels=2):
    """-> (eps, the rounds refine_adaptive yielded, {level: render(ns = level)})"""
    ks = ar.rounds_of(first, chunk, cap)
    errs = _uniform(ds, nx, ny, ks, precision, region)
    eps = _choose_eps(errs, nx, ny, first, region) if eps is None else eps
    rounds = ar.schedule(lambda k: _full(errs[k], nx, ny, region), nx, ny, first, chunk, cap, eps, region)
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    local = np.zeros(rounds[0][2].shape, bool)  # the frame's local tiles: those that meet the region
    local[y0 // 8:(y1 + 7) // 8, x0 // 8:(x1 + 7) // 8] = True
    got = []
    for g, (_, _, act, _) in zip(ds.refine_adaptive(nx, ny, cap, chunk, eps, first=first, precision=precision, region=region), rounds):
        got.append(g)  # the active list after every round: the tiles still active, in ascending tile order
        assert np.array_equal(ds.ctx.adaptive_active_tiles(), np.flatnonzero((act & local).ravel())), (g[0], "active list")
    assert [g[0] for g in got] == [k for k, _, _, _ in rounds]
    for (k, lin, q, err, spp, cnt, active), (_, n_t, act, _) in zip(got, rounds):
        assert np.array_equal(spp, _crop(ar.per_pixel(n_t, nx, ny), region)), (k, "samples per pixel")
        assert active == int((act & local).sum()), k
    k, lin, q, err, spp, cnt, active = got[-1]
    levels = [int(n) for n in np.unique(spp)]
    assert len(levels) >= min_levels, levels
    one = {}
    for n in levels:
        one[n] = ds.render(nx, ny, n, precision=precision, region=region)  # (the frame keeps its own tile lists: this does not disturb it)
        m = spp == n
        assert lin[m].tobytes() == one[n][0][m].tobytes() and np.array_equal(q[m], one[n][1][m]), (n, "against render(ns = %d)" % n)
        assert err[m].tobytes() == errs[n][m].tobytes(), (n, "out_stderr against the uniform run's plane")
    assert ds.ctx.adaptive_status()[2] == int(spp.sum()) and int(cnt[1]) == spp.size
    return eps, got, one


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_cover_against_one_shot(cover, precision):
    _check_against_uniform(cover, 200, 100, 8, 8, 32, precision)


def test_cornell_box_tree_and_flat_scan(ctx):
    ds = core.DeviceScene(r.scene.make_cornell_box(64, 64), ctx=ctx)
    try:
        eps, tree, _ = _check_against_uniform(ds, 64, 64, 8, 8, 32)
        assert ctx.last_accel() == "bvh"
        ctx.set_option("accel", 0)
        try:
            _, flat, _ = _check_against_uniform(ds, 64, 64, 8, 8, 32, eps=eps)
            assert ctx.last_accel() == "flat"
        finally:
            ctx.set_option("accel", 1)
        assert _same(tree[-1][1:6], flat[-1][1:6])
    finally:
        ds.close()


def test_make_final_against_one_shot(ctx):
    ds = core.DeviceScene(r.scene.make_final(64, 64), ctx=ctx)  # media draws, Perlin, image texture
    try:
        _check_against_uniform(ds, 64, 64, 8, 8, 32)
    finally:
        ds.close()


def test_region_against_one_shot_with_counters(cover):
    nx, ny = 200, 100
    x0, y0, x1, y1 = REGION
    eps, got, _ = _check_against_uniform(cover, nx, ny, 4, 4, 16, region=REGION)
    spp, cnt = got[-1][4], got[-1][5]
    rays = 0
    for ty in range(y0 // 8, (y1 + 7) // 8):
        for tx in range(x0 // 8, (x1 + 7) // 8):
            tile = (max(tx * 8, x0), max(ty * 8, y0), min(tx * 8 + 8, x1), min(ty * 8 + 8, y1))
            n = int(spp[tile[1] - y0, tile[0] - x0])
            assert (spp[tile[1] - y0:tile[3] - y0, tile[0] - x0:tile[2] - x0] == n).all()
            rays += int(cover.render(nx, ny, n, region=tile)[2][0])
    assert int(cnt[0]) == rays and int(cnt[1]) == (x1 - x0) * (y1 - y0)


# ---- the edges of eps -------------------------------------------------------------------------------------------------------------------------
def test_eps_zero_on_a_constant_world(ctx):
    ds = core.DeviceScene(fr.constant_light_scene((0.3, 0.7, 1.9)), ctx=ctx)
    nx, ny = 32, 16
    try:
        lin, q, err, spp, cnt = ds.render_adaptive(nx, ny, 0, 1, 0.0)  # k = 1: nothing can retire
        assert np.isinf(err).all() and (spp == 1).all() and ctx.adaptive_status() == (8, 8, nx * ny)
        lin, q, err, spp, cnt = ds.render_adaptive(nx, ny, 0, 2, 0.0)  # a new frame; all samples equal: every tile retires after round one
        assert (err == 0).all() and (spp == 2).all() and int(cnt[0]) == nx * ny * 2
        assert ctx.adaptive_status() == (0, 8, nx * ny * 2)
        again = ds.render_adaptive(nx, ny, 2, 3, 0.0)  # traces nothing
        assert _same(again, (lin, q, err, spp, cnt))
        assert ctx.adaptive_status() == (0, 8, nx * ny * 2) and ctx.progressive_samples() == 5
        assert _same(ds.render(nx, ny, 2)[:2], (lin, q))
        assert [g[0] for g in ds.refine_adaptive(nx, ny, 64, 4, 0.0)] == [4]
    finally:
        ds.close()
        ctx.progressive_release()


def test_huge_eps_and_tiny_eps(ctx, cover):
    nx, ny = 200, 100
    got = list(cover.refine_adaptive(nx, ny, 16, 4, 1e30, first=3))
    assert [g[0] for g in got] == [3] and got[0][6] == 0 and (got[0][4] == 3).all()
    one = cover.render(nx, ny, 3)
    assert _same((got[0][1], got[0][2], got[0][5]), one)
    got = list(cover.refine_adaptive(nx, ny, 16, 4, 1e-9, first=3))
    total = ctx.adaptive_status()[1]
    assert [g[0] for g in got] == [3, 7, 11, 15, 16] and all(g[6] == total for g in got)  # nothing retires: the input this case needs
    one = cover.render(nx, ny, 16)
    assert _same((got[-1][1], got[-1][2], got[-1][5]), one) and (got[-1][4] == 16).all()
    assert ctx.adaptive_status() == (total, total, nx * ny * 16)


# ---- invariance -------------------------------------------------------------------------------------------------------------------------------
def _eps_for(cover, first, chunk, cap):
    errs = _uniform(cover, 200, 100, ar.rounds_of(first, chunk, cap))
    return _choose_eps(errs, 200, 100, first)


def test_sample_passes_interleaved_renders_and_accel_switch(ctx, cover):
    nx, ny = 200, 100
    eps = _eps_for(cover, 4, 4, 16)
    base = list(cover.refine_adaptive(nx, ny, 16, 4, eps))
    assert len(np.unique(base[-1][4])) >= 2 and 0 < base[0][6] < ctx.adaptive_status()[1]
    ctx.set_option("workspace_bytes", 1 << 20)  # several passes per round
    try:
        it = cover.refine_adaptive(nx, ny, 16, 4, eps)
        small = [next(it)]
        assert _passes(ctx) >= 2
        small += list(it)
    finally:
        ctx.set_option("workspace_bytes", 8 << 30)
    assert all(_same(a[1:], b[1:]) for a, b in zip(base, small)) and len(base) == len(small)
    mixed = []
    other = core.DeviceScene(r.scene.make_random_scene(96, 40, 3, False), ctx=ctx)
    try:
        for g in cover.refine_adaptive(nx, ny, 16, 4, eps):
            mixed.append(g)
            other.render(96, 40, 6)  # another size on the same context rewrites the context's tile list, not the frame's
            ctx.set_option("accel", len(mixed) % 2)
    finally:
        ctx.set_option("accel", 1)
        other.close()
    assert all(_same(a[1:], b[1:]) for a, b in zip(base, mixed)) and len(base) == len(mixed)


def test_frame_started_by_render_progressive(ctx, cover):
    nx, ny = 200, 100
    eps = _eps_for(cover, 4, 4, 16)
    base = [cover.render_adaptive(nx, ny, 0, 4, 0.0)]  # eps may change between calls: nothing retires in this round
    total = ctx.adaptive_status()[1]
    assert ctx.adaptive_status() == (total, total, nx * ny * 4)
    base += [cover.render_adaptive(nx, ny, k, 4, eps) for k in (4, 8, 12)]
    status = ctx.adaptive_status()
    assert len(np.unique(base[-1][3])) >= 2
    lin, q, err, cnt = cover.render_progressive(nx, ny, 0, 4)
    assert _same((lin, q, err, cnt), (base[0][0], base[0][1], base[0][2], base[0][4]))
    assert ctx.adaptive_status() == (total, total, nx * ny * 4)  # the special case: every tile active with n_t = k
    cont = [cover.render_adaptive(nx, ny, k, 4, eps) for k in (4, 8, 12)]
    assert all(_same(a, b) for a, b in zip(base[1:], cont)) and ctx.adaptive_status() == status
    # an adaptive frame in which nothing has retired is still a uniform frame: render_progressive may continue it
    cover.render_adaptive(nx, ny, 0, 4, 0.0)
    lin, q, err, cnt = cover.render_progressive(nx, ny, 4, 3)
    assert _same((lin, q, cnt), cover.render(nx, ny, 7))
    spp = cover.render_adaptive(nx, ny, 7, 1, 0.0)[3]
    assert (spp == 8).all()


# ---- state errors -----------------------------------------------------------------------------------------------------------------------------
def _call(ds, nx, ny, s_first, s_count, eps, depth=50, seed=core.RENDER_SEED, precision=0, region=None):
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    return r._ffi.lib().rtmi_render_adaptive(ds.handle, nx, ny, s_first, s_count, eps, depth, seed, precision, x0, y0, x1, y1,
                                             None, None, None, None, None)


def test_state_errors_leave_the_frame(ctx, cover):
    L = r._ffi.lib()
    nx, ny = 200, 100
    eps = _eps_for(cover, 4, 4, 12)
    base = list(cover.refine_adaptive(nx, ny, 12, 4, eps))
    first = cover.render_adaptive(nx, ny, 0, 4, eps)
    status = ctx.adaptive_status()
    assert 0 < status[0] < status[1]  # tiles have retired
    # rtmi_render_progressive cannot continue it
    rc = L.rtmi_render_progressive(cover.handle, nx, ny, 4, 4, 50, core.RENDER_SEED, 0, 0, 0, nx, ny, None, None, None, None)
    assert rc == RTMI_E_STATE and "retired" in L.rtmi_last_error().decode()
    rc = L.rtmi_render_progressive_device(cover.handle, nx, ny, 4, 4, 50, core.RENDER_SEED, 0, None, None, None, None, None)
    assert rc == RTMI_E_STATE and "retired" in L.rtmi_last_error().decode()
    assert ctx.adaptive_status() == status and ctx.progressive_samples() == 4
    # key mismatches and a wrong s_first
    bad = [dict(s_first=3), dict(s_first=8), dict(seed=core.RENDER_SEED + 1), dict(depth=49), dict(nx=208), dict(precision=1),
           dict(region=(0, 0, 100, 100))]
    for kw in bad:
        args = dict(nx=nx, ny=ny, s_first=4, s_count=4)
        args.update(kw)
        a, b, s_first, s_count = args.pop("nx"), args.pop("ny"), args.pop("s_first"), args.pop("s_count")
        assert _call(cover, a, b, s_first, s_count, eps, **args) == RTMI_E_STATE, kw
        assert L.rtmi_last_error().decode(), kw
        assert ctx.adaptive_status() == status and ctx.progressive_samples() == 4, kw
    for e in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert _call(cover, nx, ny, 4, 4, e) == RTMI_E_ARG and "eps" in L.rtmi_last_error().decode(), e
        assert _call(cover, nx, ny, 0, 4, e) == RTMI_E_ARG, e
    assert ctx.adaptive_status() == status and ctx.progressive_samples() == 4
    ctx.set_option("test_fail_next_render", 1)
    with pytest.raises(r._ffi.RtmiError):
        cover.render_adaptive(nx, ny, 4, 4, eps)
    assert ctx.adaptive_status() == status and ctx.progressive_samples() == 4  # failed before launching anything
    rest = [cover.render_adaptive(nx, ny, k, 4, eps) for k in (4, 8)]
    assert _same(first, base[0][1:6]) and all(_same(a, b[1:6]) for a, b in zip(rest, base[1:]))
    ctx.progressive_release()
    assert ctx.adaptive_status() == (0, 0, 0) and ctx.progressive_samples() == 0
    assert _call(cover, nx, ny, 12, 4, eps) == RTMI_E_STATE
    fresh = core.Context(0)
    try:
        assert fresh.adaptive_status() == (0, 0, 0)
        ds = core.DeviceScene(r.scene.make_random_scene(64, 32, 3, False), ctx=fresh)
        assert _call(ds, 64, 32, 2, 2, 0.1) == RTMI_E_STATE and fresh.adaptive_status() == (0, 0, 0)  # s_first > 0 without a frame
        ds.close()
    finally:
        fresh.close()


def test_timing_flag_covers_adaptive_calls():
    timed = core.Context(0, timing=True)
    try:
        ds = core.DeviceScene(r.scene.make_random_scene(200, 100, 11, True), ctx=timed)
        rounds = list(ds.refine_adaptive(200, 100, 12, 4, 1e-9))
        assert len(rounds) == 3
        ms, launches = timed.last_trace_ms()
        assert launches == 3 and ms > 0  # one trace launch per round (one pass each)
        rms, folds = timed.last_reduce_ms()
        assert folds == 3 and rms > 0  # the "reduce" interval of an adaptive pass is its fold
        ds.close()
    finally:
        timed.close()


# ---- device form ------------------------------------------------------------------------------------------------------------------------------
def test_device_form_matches_host_form(ctx, cover):
    import torch
    nx, ny = 200, 100
    eps = _eps_for(cover, 4, 4, 12)
    host = [cover.render_adaptive(nx, ny, k, 4, eps) for k in (0, 4, 8)]
    status = ctx.adaptive_status()
    assert len(np.unique(host[-1][3])) >= 2
    lin = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
    q = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
    err = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    spp = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    for k, h in zip((0, 4, 8), host):
        cover.render_adaptive_device(nx, ny, k, 4, eps, lin, q, err, spp, cnt)
        torch.cuda.synchronize()
        got = (lin.cpu().numpy(), q.cpu().numpy(), err.cpu().numpy(), spp.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64))
        assert _same(got, h), k
    assert ctx.adaptive_status() == status
    cover.render_adaptive_device(nx, ny, 12, 1, eps)  # every output may be NULL
    torch.cuda.synchronize()
    assert ctx.progressive_samples() == 13 and ctx.adaptive_status()[0] <= status[0]


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def _progress_lines(text):
    return [l for l in text.splitlines() if re.fullmatch(r"\d+\.\d\ds, \d+%, ETA -?\d+\.\d\ds", l)]


def test_cli_adaptive(tmp_path, capsys):
    head = b"P6\n64 32\n255\n"
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"
    assert core.main([str(a), "64", "32", "10"]) == 0
    capsys.readouterr()
    assert core.main([str(b), "64", "32", "10", "--adaptive", "1e-9", "--chunk", "4"]) == 0  # nothing retires: the plain run's file
    text = capsys.readouterr().out
    assert a.read_bytes() == b.read_bytes()
    assert len(_progress_lines(text)) == 3 and "samples: mean 10.00 of 10 per pixel, 0 of 32 tiles converged" in text
    assert core.main([str(b), "64", "32", "10", "--adaptive", "1e9", "--chunk", "4"]) == 0  # everything retires after round one
    text = capsys.readouterr().out
    assert len(_progress_lines(text)) == 1 and "samples: mean 4.00 of 10 per pixel, 32 of 32 tiles converged" in text
    ds = core.DeviceScene(r.scene.make_random_scene(64, 32, 11, True))
    try:
        _, q4, cnt4 = ds.render(64, 32, 4)
        img = np.frombuffer(b.read_bytes()[len(head):], np.uint8).reshape(32, 64, 3)
        assert np.array_equal(img, q4) and ("total-rays %d " % int(cnt4[0])) in text
        # an eps in between: the file is the per-tile composition of one-shot renders
        errs = _uniform(ds, 64, 32, ar.rounds_of(16, 16, 64))
        eps = _choose_eps(errs, 64, 32, 16)
        got = list(ds.refine_adaptive(64, 32, 64, 16, eps))
        spp = got[-1][4]
        assert len(np.unique(spp)) >= 2
        assert core.main([str(b), "64", "32", "64", "--adaptive", repr(eps)]) == 0  # rounds of 16 by default
        text = capsys.readouterr().out
        img = np.frombuffer(b.read_bytes()[len(head):], np.uint8).reshape(32, 64, 3)
        for n in np.unique(spp):
            assert np.array_equal(img[spp == n], ds.render(64, 32, int(n))[1][spp == n]), n
        assert ("samples: mean %.2f of 64 per pixel, %d of 32 tiles converged" % (spp.mean(), 32 - got[-1][6])) in text
        assert len(_progress_lines(text)) == len(got)
    finally:
        ds.ctx.progressive_release()
        ds.close()


# ---- one frame at C3 size -----------------------------------------------------------------------------------------------------------------------
def test_c3_frame_per_level(ctx):
    nx, ny = 1920, 1080
    ds = core.DeviceScene(r.scene.make_random_scene(nx, ny, 50, False, mix=(0.8, 0.95)), ctx=ctx)
    try:
        _check_against_uniform(ds, nx, ny, 64, 64, 256, min_levels=4)  # 64, 128, 192 and 256: four one-shot renders
    finally:
        ds.close()
        ctx.progressive_release()
