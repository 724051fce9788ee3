"""Progressive rendering on the device (rtmi_render_progressive*): after every chunk the frame is bit for bit the one-shot render with ns = k,
whatever the chunks, the sample passes inside a call, the one-shot renders and option changes in between; continuations with another key are
refused and leave the frame alone; the per-pixel noise estimate is exact where it can be and agrees with numpy elsewhere."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import hitable as hitm
from raytrace_clj_amd import shader as shad
from raytrace_clj_amd import texture as texm
from raytrace_clj_amd.util import vec3

pytestmark = pytest.mark.gpu

RTMI_E_STATE, RTMI_E_UNSUPPORTED = -5, -3


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_chunks(ds, nx, ny, chunks, precision="f64", region=None):
    """every chunk's (linear, rgb8, counters) against the one-shot render with ns = k; -> the last progressive result"""
    k, last = 0, None
    for n in chunks:
        lin, q, err, cnt = ds.render_progressive(nx, ny, k, n, precision=precision, region=region)
        k += n
        assert ds.ctx.progressive_samples() == k
        elin, eq, ecnt = ds.render(nx, ny, k, precision=precision, region=region)
        assert np.array_equal(lin, elin) and np.array_equal(q, eq) and np.array_equal(cnt, ecnt), (precision, k)
        assert err.shape == lin.shape[:2] and (np.isinf(err).all() if k == 1 else np.isfinite(err).all())
        last = (lin, q, err, cnt)
    return last


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


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_cover_chunks_bit_identical(cover, precision):
    _check_chunks(cover, 200, 100, [1, 3, 4, 8], precision)


def test_cornell_box_tree_and_flat_scan_bit_identical(ctx):
    ds = core.DeviceScene(r.scene.make_cornell_box(64, 64), ctx=ctx)
    try:
        _check_chunks(ds, 64, 64, [2, 3, 5])
        assert ctx.last_accel() == "bvh"
        ctx.set_option("accel", 0)  # the flat scan: the SCAN_SGPR_CULL mixed-kind kernel option flat_below selects
        try:
            _check_chunks(ds, 64, 64, [2, 3, 5])
            assert ctx.last_accel() == "flat"
        finally:
            ctx.set_option("accel", 1)
        L = r._ffi.lib()
        k = ctx.progressive_samples()
        lin = np.zeros((64, 64, 3))
        rc = L.rtmi_render_progressive(ds.handle, 64, 64, 0, 1, 50, core.RENDER_SEED, 1, 0, 0, 64, 64, r._ffi.ptr(lin), None, None, None)
        assert rc == RTMI_E_UNSUPPORTED and ctx.progressive_samples() == k  # F32 on a mixed-kind scene: rtmi_render's answer, frame untouched
        cnt = np.zeros(2, np.uint64)
        assert L.rtmi_render(ds.handle, 64, 64, 1, 50, core.RENDER_SEED, 1, 0, 0, 64, 64, None, None, r._ffi.ptr(cnt)) == RTMI_E_UNSUPPORTED
    finally:
        ds.close()


def test_make_final_bit_identical(ctx):
    ds = core.DeviceScene(r.scene.make_final(64, 64), ctx=ctx)  # media draws, Perlin, image texture
    try:
        _check_chunks(ds, 64, 64, [1, 2, 5])
    finally:
        ds.close()


def test_region_bit_identical(cover):
    _check_chunks(cover, 200, 100, [2, 3, 3], region=(37, 21, 101, 59))


def test_sample_passes_inside_a_call(ctx, cover):
    lin0, q0, _, cnt0 = _check_chunks(cover, 200, 100, [3, 5, 4])
    ctx.set_option("workspace_bytes", 1 << 20)  # two samples per pass: boundaries 0, 2, 4, ... against chunk boundaries 3, 8
    try:
        lin, q, _, cnt = _check_chunks(cover, 200, 100, [3, 5, 4])
        passes = C.c_int32()
        core.check(r._ffi.lib().rtmi_last_passes(ctx.handle, C.byref(passes)))
        assert passes.value >= 2
    finally:
        ctx.set_option("workspace_bytes", 8 << 30)
    assert _same((lin, q, cnt), (lin0, q0, cnt0))


def test_interleaved_one_shot_render_and_accel_switch(ctx, cover):
    ref = cover.render(200, 100, 12)
    cover.render_progressive(200, 100, 0, 4)
    other = core.DeviceScene(r.scene.make_random_scene(96, 40, 3, False), ctx=ctx)
    try:
        other.render(96, 40, 6)  # another size on the same context: its workspace, not the frame
    finally:
        other.close()
    ctx.set_option("accel", 0)
    try:
        cover.render_progressive(200, 100, 4, 4)
    finally:
        ctx.set_option("accel", 1)
    lin, q, _, cnt = cover.render_progressive(200, 100, 8, 4)
    assert _same((lin, q, cnt), ref)


def test_device_form_matches_host_form(ctx, cover):
    import torch
    nx, ny = 200, 100
    host = [cover.render_progressive(nx, ny, 0, 3), cover.render_progressive(nx, ny, 3, 2)]
    lin = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
    q = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
    err = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    for (k0, n), h in zip([(0, 3), (3, 2)], host):
        cover.render_progressive_device(nx, ny, k0, n, lin, q, err, cnt)
        torch.cuda.synchronize()
        got = (lin.cpu().numpy(), q.cpu().numpy(), err.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, h))
    cover.render_progressive_device(nx, ny, 5, 1)  # every output may be NULL
    torch.cuda.synchronize()
    assert ctx.progressive_samples() == 6


def _call(ds, nx, ny, s_first, s_count, depth=50, seed=core.RENDER_SEED, precision=0, region=None):
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    return r._ffi.lib().rtmi_render_progressive(ds.handle, nx, ny, s_first, s_count, depth, seed, precision, x0, y0, x1, y1, None, None, None, None)


def test_state_errors_leave_the_frame(ctx, cover):
    L = r._ffi.lib()
    fresh = core.Context(0)
    try:
        ds = core.DeviceScene(r.scene.make_random_scene(64, 32, 3, False), ctx=fresh)
        assert _call(ds, 64, 32, 2, 2) == RTMI_E_STATE and L.rtmi_last_error()  # s_first > 0 without a frame
        assert fresh.progressive_samples() == 0
        ds.close()
    finally:
        fresh.close()
    assert _call(cover, 200, 100, 0, 3) == 0
    bad = [dict(s_first=2), dict(s_first=4), dict(seed=core.RENDER_SEED + 1), dict(depth=49), dict(nx=208), dict(precision=1),
           dict(region=(0, 0, 100, 100))]
    for kw in bad:
        args = dict(nx=200, ny=100, s_first=3, s_count=2)
        args.update(kw)
        nx, ny, s_first, s_count = args.pop("nx"), args.pop("ny"), args.pop("s_first"), args.pop("s_count")
        assert _call(cover, nx, ny, s_first, s_count, **args) == RTMI_E_STATE, kw
        assert L.rtmi_last_error().decode(), kw
        assert ctx.progressive_samples() == 3, kw
    # another scene, then the same scene's world re-created after the frame's scene was destroyed (possibly at the same address)
    twin = core.DeviceScene(cover.flat, ctx=ctx)
    assert _call(twin, 200, 100, 3, 2) == RTMI_E_STATE and ctx.progressive_samples() == 3
    twin.close()
    ds = core.DeviceScene(cover.flat, ctx=ctx)
    assert _call(ds, 200, 100, 0, 3) == 0
    flat = ds.flat
    ds.close()
    again = core.DeviceScene(flat, ctx=ctx)
    try:
        assert _call(again, 200, 100, 3, 2) == RTMI_E_STATE and ctx.progressive_samples() == 3
        # the same scene after rtmi_scene_set_perlin (any rtmi_scene_set_* call changes the scene's revision)
        assert _call(again, 200, 100, 0, 3) == 0
        rng = np.random.default_rng(5)
        vec = rng.normal(size=(256, 3))
        vec /= np.linalg.norm(vec, axis=1, keepdims=True)
        perm = np.concatenate([rng.permutation(256) for _ in range(3)]).astype(np.int32)
        core.check(L.rtmi_scene_set_perlin(again.handle, r._ffi.ptr(np.ascontiguousarray(vec)), r._ffi.ptr(perm)))
        assert _call(again, 200, 100, 3, 2) == RTMI_E_STATE and ctx.progressive_samples() == 3
        assert "changed" in L.rtmi_last_error().decode()
    finally:
        again.close()


def test_failed_continuation_recovers_and_release(ctx, cover):
    cover.render_progressive(200, 100, 0, 3)
    ctx.set_option("test_fail_next_render", 1)
    with pytest.raises(r._ffi.RtmiError):
        cover.render_progressive(200, 100, 3, 4)
    assert ctx.progressive_samples() == 3  # failed before launching anything: the frame is as it was
    lin, q, _, cnt = cover.render_progressive(200, 100, 3, 4)
    assert _same((lin, q, cnt), cover.render(200, 100, 7))
    core.check(r._ffi.lib().rtmi_progressive_release(ctx.handle))
    assert ctx.progressive_samples() == 0
    assert _call(cover, 200, 100, 7, 1) == RTMI_E_STATE


def test_noise_estimate_exact_for_a_constant_world(ctx):
    camera = r.camera.pinhole_camera(lookfrom=vec3(0, 0, 0), lookat=vec3(0, 0, -1), vup=vec3(0, 1, 0), vfov=90, aspect=2.0)
    light = shad.diffuse_light(tex=texm.constant(color=vec3(0.3, 0.7, 1.9)))
    ds = core.DeviceScene(hitm.Hitlist([hitm.sphere(center=vec3(0, 0, 0), radius=100.0, material=light)]), camera, ctx=ctx)
    try:
        for k, lin, q, err, cnt in ds.refine(32, 16, 6, 1):
            assert np.allclose(lin, [0.3, 0.7, 1.9], rtol=1e-15, atol=0)
            assert np.isinf(err).all() if k == 1 else (err == 0).all()
            assert int(cnt[0]) == 32 * 16 * k  # one segment per sample
    finally:
        ds.close()


def test_noise_estimate_against_numpy(cover):
    means = [np.zeros((100, 200, 3))]
    errs = [None]
    for k, lin, q, err, cnt in cover.refine(200, 100, 8, 1):
        means.append(lin)
        errs.append(err)
    x = np.stack([(j + 1) * means[j + 1] - j * means[j] for j in range(8)])  # the sample values, from consecutive means
    for k in (2, 5, 8):
        ref = np.sqrt(x[:k].var(axis=0, ddof=1) / k).max(axis=2)
        sel = ref > 1e-9
        assert sel.mean() > 0.5
        np.testing.assert_allclose(errs[k][sel], ref[sel], rtol=1e-6, atol=1e-12)


def test_c3_four_chunks_of_64(ctx):
    nx, ny = 1920, 1080
    ds = core.DeviceScene(r.scene.make_random_scene(nx, ny, 50, False, mix=(0.8, 0.95)), ctx=ctx)
    try:
        ref = ds.render(nx, ny, 256)
        for k, lin, q, err, cnt in ds.refine(nx, ny, 256, 64):
            pass
        assert k == 256 and _same((lin, q, cnt), ref)
    finally:
        ds.close()
        ctx.progressive_release()


def _progress_lines(text):
    return [l for l in text.splitlines() if re.fullmatch(r"\d+\.\d\ds, \d+%, ETA -?\d+\.\d\ds", l)]


def test_cli_chunks(tmp_path, capsys):
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"
    assert core.main([str(a), "64", "32", "10"]) == 0
    capsys.readouterr()
    assert core.main([str(b), "64", "32", "10", "--chunk", "4"]) == 0
    out = capsys.readouterr().out
    assert a.read_bytes() == b.read_bytes()
    assert len(_progress_lines(out)) == math.ceil(10 / 4) and "100%" in _progress_lines(out)[-1]


def test_cli_budget_and_noise_stop_early(tmp_path, capsys):
    head = b"P6\n64 32\n255\n"
    out = tmp_path / "b.ppm"
    assert core.main([str(out), "64", "32", "10", "--chunk", "4", "--budget", "0"]) == 0
    text = capsys.readouterr().out
    assert len(_progress_lines(text)) == 1 and "stopped at 4 of 10" in text
    img = np.frombuffer(out.read_bytes()[len(head):], np.uint8).reshape(32, 64, 3)
    ds = core.DeviceScene(r.scene.make_random_scene(64, 32, 11, True))
    try:
        _, q, cnt = ds.render(64, 32, 4)
    finally:
        ds.close()
    assert np.array_equal(img, q) and ("total-rays %d " % int(cnt[0])) in text
    assert core.main([str(out), "64", "32", "10", "--chunk", "1", "--noise", "1e9"]) == 0
    text = capsys.readouterr().out
    assert len(_progress_lines(text)) == 2 and "stopped at 2 of 10" in text
