"""Adaptive sampling steered by the denoised frame's noise estimate on the device: rtmi_adaptive_retire* retires tiles by a map the caller
supplies, DeviceScene.refine_adaptive_denoised closes the loop render_adaptive -> denoise -> adaptive_retire.

  * libm-free scenes, the cases of adaptive_denoised_reference.py: after every round the samples per pixel, the active list, the frame, the
    ray counter, the filtered frame and its standard error equal what numpy derives from the oracle's individual samples.
  * rtmi_adaptive_retire on hand-made maps (exactly eps, the next double, NaN, +-inf, partial tiles at the right and bottom edge, a region that
    cuts tiles, bad pixels outside the region), a frame of more than 1024 tiles, scenes that use libm against the library's own one-shot
    render with the retirements recomputed in numpy from the very map the call was handed.
  * state and argument errors leave the frame alone; device form = host form; interleaved calls and sample passes: same bytes; the CLI; and on
    the Cornell box the loop takes fewer samples than the uniform run and ends closer to the truth than the 16-spp frame it starts from.

Every comparison below is an equality, except the two inequalities of test_it_pays_on_the_cornell_box."""
import ctypes as C

import numpy as np
import pytest

import adaptive_denoised_reference as adr
import adaptive_reference as ar
import denoise_reference as dr
import frame_reference as fr
import raytrace_clj_amd as r
from raytrace_clj_amd import core

pytestmark = pytest.mark.gpu

RTMI_E_ARG, RTMI_E_STATE = -1, -5
EPS_MAPS = 0.25


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


def _same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _mask(ctx, nx, ny):
    """the frame's active list as [tiles_y, tiles_x] bool; the list itself must be ascending"""
    tx, ty = fr.tiles_of(nx, ny)
    tiles = ctx.adaptive_active_tiles()
    assert tiles.dtype == np.int32 and (np.diff(tiles) > 0).all()
    m = np.zeros(ty * tx, bool)
    m[tiles] = True
    return m.reshape(ty, tx)


def _choose_eps(ferr):
    """midway inside the widest (relative) gap of the sorted per-tile maxima of a filtered noise plane, looked for in the middle half (as
    test_gpu_adaptive.py chooses its eps from the raw plane)"""
    v = np.unique(ar.tile_max(ferr))
    v = v[np.isfinite(v) & (v > 0)]
    assert len(v) >= 8, "too few distinct per-tile maxima to choose from"
    lo, hi = len(v) // 4, 3 * len(v) // 4
    i = lo + int(np.argmax(v[lo + 1:hi + 1] / v[lo:hi]))
    return float(0.5 * (v[i] + v[i + 1]))


def _eps_from_first_round(ds, nx, ny, first, **kw):
    """eps for a run of refine_adaptive_denoised, from the filtered noise plane of its first round"""
    try:
        g = next(ds.refine_adaptive_denoised(nx, ny, first, first, 0.0, **kw))
    finally:
        ds.ctx.progressive_release()
    return _choose_eps(g[9])


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cover(ctx):
    ds = core.DeviceScene(r.scene.make_random_scene(200, 100, 11, True), ctx=ctx)
    yield ds
    ctx.progressive_release()
    ds.close()


# ---- 1. the oracle and the numpy filter, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", adr.CASES, ids=ar.case_id)
def test_oracle_schedule_frames_and_filter(request, ctx, case):
    name, precision, (nx, ny), first, chunk, cap, eps = case
    o = _oracle(request, precision)
    smp, nseg, feat, rounds = adr.reference_run(o, case)
    ds = core.DeviceScene(fr.scene(name, nx, ny), ctx=ctx)
    try:
        got, lists = [], []
        for g in ds.refine_adaptive_denoised(nx, ny, cap, chunk, eps, first=first, na=adr.NA, precision=precision, depth=fr.DEPTH, seed=fr.SEED):
            got.append(g)
            lists.append(ctx.adaptive_active_tiles())  # the list the next round traces
        assert [g[0] for g in got] == [m["k"] for m in rounds]
        for (k, lin, q, err, spp, cnt, active, flt, fq, ferr), m, tiles in zip(got, rounds, lists):
            n_px = ar.per_pixel(m["n_t"], nx, ny)
            assert spp.dtype == np.int32 and np.array_equal(spp, n_px), (k, "samples per pixel")
            assert active == int(m["active"].sum()), (k, active, int(m["active"].sum()))
            assert tiles.dtype == np.int32 and np.array_equal(tiles, np.flatnonzero(m["active"].ravel())), (k, "active list")
            assert np.array_equal(lin, m["linear"]), (k, "linear: %d pixels differ" % (lin != m["linear"]).any(axis=2).sum())
            assert np.array_equal(q, fr.quantise(m["linear"])), (k, "rgb8")
            assert int(cnt[0]) == ar.expected_rays(nseg, n_px) and int(cnt[1]) == nx * ny, (k, cnt)
            assert err.tobytes() == m["stderr"].tobytes(), (k, "stderr: %d pixels differ" % (err != m["stderr"]).sum())
            assert flt.tobytes() == m["flt_linear"].tobytes(), (k, "filtered: %d pixels differ" % (flt != m["flt_linear"]).any(axis=2).sum())
            assert ferr.tobytes() == m["flt_stderr"].tobytes(), (k, "filtered stderr: %d pixels differ" % (ferr != m["flt_stderr"]).sum())
            assert np.array_equal(fq, m["flt_rgb8"]), (k, "filtered rgb8")
        last = rounds[-1]
        assert ctx.adaptive_status() == (int(last["active"].sum()), last["active"].size, int(ar.per_pixel(last["n_t"], nx, ny).sum()))
        assert ctx.progressive_samples() == cap
    finally:
        ds.close()
        ctx.progressive_release()


# ---- 2. rtmi_adaptive_retire on hand-made maps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,region", [((61, 37), None), ((203, 99), adr.REGION)], ids=["61x37", "203x99-region"])
def test_retire_on_hand_made_maps(ctx, size, region):
    nx, ny = size
    kw = dict(depth=fr.DEPTH, seed=fr.SEED, region=region)
    ds = core.DeviceScene(fr.scene("spheres", nx, ny), ctx=ctx)
    local = adr.local_tiles(nx, ny, region)
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    valid = (x1 - x0) * (y1 - y0)
    try:
        frame0 = ds.render_adaptive(nx, ny, 0, 2, 0.0, **kw)
        before = _mask(ctx, nx, ny)  # (eps = 0 has retired the tiles whose two samples are equal everywhere, if any)
        assert not (before & ~local).any() and before.sum() > 0.8 * local.sum()
        maps = adr.synthetic_maps(nx, ny, EPS_MAPS, region)
        for i, (what, m, want) in enumerate(maps):
            if i % 2:  # a frame started by render_progressive: every tile active
                ds.render_progressive(nx, ny, 0, 2, **kw)
                start = local
            else:
                ds.render_adaptive(nx, ny, 0, 2, 0.0, **kw)
                start = before
            want = want & start
            assert np.array_equal(want, adr.retire(start.copy(), m, EPS_MAPS, region)), what
            retired = ctx.adaptive_retire(m, EPS_MAPS)
            assert np.array_equal(_mask(ctx, nx, ny), want), (what, "active list")
            assert retired == int(start.sum() - want.sum()), (what, retired)
            assert ctx.adaptive_status() == (int(want.sum()), int(local.sum()), valid * 2) and ctx.progressive_samples() == 2, what
            assert ctx.adaptive_retire(m, EPS_MAPS) == 0, (what, "a second identical call retires nothing")
            assert np.array_equal(_mask(ctx, nx, ny), want), what
            if not want.any():  # everything has retired: nothing is launched, whatever the map holds
                assert ctx.adaptive_retire(np.full((ny, nx), np.nan), EPS_MAPS) == 0 and ctx.adaptive_status()[0] == 0, what
                again = ds.render_adaptive(nx, ny, 2, 2, 0.0, **kw)  # no tile takes a sample: the frame of the first two
                assert _same(again, frame0), what
                assert (again[3] == 2).all() and _same(again[:2], ds.render(nx, ny, 2, fr.DEPTH, fr.SEED, region=region)[:2]), what
        assert sum(1 for _, _, w in maps if not w.any()) >= 1
        # the frame is otherwise untouched: the next round samples exactly the tiles still active, and every level is the one-shot render
        what, m, want = maps[4]
        assert what.startswith("one bad pixel per tile")
        ds.render_adaptive(nx, ny, 0, 2, 0.0, **kw)
        want = want & before
        assert ctx.adaptive_retire(m, EPS_MAPS) == int(before.sum() - want.sum())
        lin, q, err, spp, cnt = ds.render_adaptive(nx, ny, 2, 2, 0.0, **kw)
        n_t = np.where(want, 4, 2)
        crop = ar.per_pixel(n_t, nx, ny)[y0:y1, x0:x1]
        assert np.array_equal(spp, crop) and len(np.unique(spp)) == 2
        for n in (2, 4):
            one = ds.render(nx, ny, n, fr.DEPTH, fr.SEED, region=region)
            assert lin[spp == n].tobytes() == one[0][spp == n].tobytes() and np.array_equal(q[spp == n], one[1][spp == n]), n
        assert ctx.adaptive_status()[2] == int(spp.sum())
    finally:
        ds.close()
        ctx.progressive_release()


# ---- 3. a frame of more than 1024 tiles: the compaction walks two strides, the retire grid is many workgroups ---------------------------------------
def test_frame_of_more_than_1024_tiles(ctx):
    nx = ny = 264
    tx, ty = fr.tiles_of(nx, ny)
    assert tx * ty == 1089
    ds = core.DeviceScene(r.scene.make_random_scene(nx, ny, 11, True), ctx=ctx)
    try:
        ds.render_adaptive(nx, ny, 0, 2, 0.0)
        before = _mask(ctx, nx, ny)
        assert before.sum() > 1024
        odd = (np.arange(tx * ty) % 2 == 1).reshape(ty, tx)  # every other tile, in list order
        m = np.where(ar.per_pixel(odd, nx, ny), 0.0, np.inf)
        retired = ctx.adaptive_retire(m, 0.0)
        want = before & ~odd
        assert retired == int((before & odd).sum()) and np.array_equal(_mask(ctx, nx, ny), want)
        assert ctx.adaptive_status() == (int(want.sum()), tx * ty, nx * ny * 2)
        lin, q, err, spp, cnt = ds.render_adaptive(nx, ny, 2, 2, 0.0)
        assert np.array_equal(spp, ar.per_pixel(np.where(want, 4, 2), nx, ny))
        for n in (2, 4):
            one = ds.render(nx, ny, n)
            assert (spp == n).sum() > nx * ny // 3
            assert lin[spp == n].tobytes() == one[0][spp == n].tobytes() and np.array_equal(q[spp == n], one[1][spp == n]), n
    finally:
        ds.close()
        ctx.progressive_release()


# ---- 4. scenes that use libm, through the driver ----------------------------------------------------------------------------------------------------
def _check_driver_against_one_shot(ds, nx, ny, first, chunk, cap, eps=None):
    """-> (eps, the rounds the driver yielded).  Per level n of out_samples the pixels equal render(ns = n); every retirement equals the
    per-tile maxima of the filtered stderr the call was handed, compared with eps in numpy (the host form hands the device these very doubles)."""
    ctx = ds.ctx
    eps = _eps_from_first_round(ds, nx, ny, first) if eps is None else eps
    ft = ds.render_features(nx, ny, core.FEATURE_SAMPLES)[0]
    tx, ty = fr.tiles_of(nx, ny)
    active = np.ones((ty, tx), bool)
    n_t = np.zeros((ty, tx), np.int64)
    got = []
    for g in ds.refine_adaptive_denoised(nx, ny, cap, chunk, eps, first=first):
        k, lin, q, err, spp, cnt, n_active, flt, fq, ferr = g
        got.append(g)
        n_t[active] = k
        assert np.array_equal(spp, ar.per_pixel(n_t, nx, ny)), (k, "samples per pixel")
        active = active & ~(ar.tile_max(err) <= 0.0)  # the raw rule at eps 0
        active = active & ~(ar.tile_max(ferr) <= eps)  # the filtered rule, on the map the call was handed
        assert np.array_equal(_mask(ctx, nx, ny), active) and n_active == int(active.sum()), (k, "retirement")
        assert _same((flt, fq, ferr), ctx.denoise(lin, err, ft)), (k, "the filtered frame is denoise of the yielded frame")
    assert got[-1][0] == cap or not active.any()
    k, lin, q, err, spp, cnt, n_active, flt, fq, ferr = got[-1]
    levels = [int(n) for n in np.unique(spp)]
    assert len(levels) >= 2, levels
    for n in levels:
        one = ds.render(nx, ny, n)  # (the frame keeps its own tile lists: this does not disturb it)
        m = spp == n
        assert lin[m].tobytes() == one[0][m].tobytes() and np.array_equal(q[m], one[1][m]), (n, "against render(ns = %d)" % n)
    assert ctx.adaptive_status() == (int(active.sum()), tx * ty, int(spp.sum()))
    ctx.progressive_release()
    return eps, got


def test_cover_scene_against_one_shot(cover):
    eps, got = _check_driver_against_one_shot(cover, 200, 100, 8, 8, 32)
    assert 0 < got[0][6] < 325, "the first round retires some tiles and leaves some"


def test_cornell_box_tree_and_flat_scan(ctx):
    ds = core.DeviceScene(r.scene.make_cornell_box(96, 96), ctx=ctx)
    try:
        eps, tree = _check_driver_against_one_shot(ds, 96, 96, 16, 16, 64)
        assert ctx.last_accel() == "bvh" and 0 < tree[0][6] < 144
        ctx.set_option("accel", 0)
        try:
            _, flat = _check_driver_against_one_shot(ds, 96, 96, 16, 16, 64, eps=eps)
            assert ctx.last_accel() == "flat"
        finally:
            ctx.set_option("accel", 1)
        assert len(tree) == len(flat) and all(_same(a[1:], b[1:]) for a, b in zip(tree, flat))
    finally:
        ds.close()
        ctx.progressive_release()


# ---- 5. state and argument errors ----------------------------------------------------------------------------------------------------------------------
def _retire(ctx, nx, ny, noise, eps, out=None):
    p = None if noise is None else noise.ctypes.data_as(C.c_void_p)
    return r._ffi.lib().rtmi_adaptive_retire(ctx.handle, nx, ny, p, eps, None if out is None else C.byref(out))


def _retire_device(ctx, nx, ny, noise, eps):
    p = None if noise is None else noise.ctypes.data_as(C.c_void_p)  # never dereferenced: the calls below fail before anything is launched
    return r._ffi.lib().rtmi_adaptive_retire_device(ctx.handle, nx, ny, p, eps, None, None)


def test_errors_leave_the_frame(ctx, cover):
    L = r._ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    nx, ny = 200, 100
    eps = _eps_from_first_round(cover, nx, ny, 4)
    base = list(cover.refine_adaptive_denoised(nx, ny, 12, 4, eps))
    assert 0 < base[0][6] < ctx.adaptive_status()[1]  # tiles have retired after the first round
    ok = np.zeros((ny, nx))

    def disturb():
        status, k, tiles = ctx.adaptive_status(), ctx.progressive_samples(), ctx.adaptive_active_tiles()
        n = C.c_int32(-7)
        for call in (_retire, _retire_device):
            assert call(ctx, nx, ny, None, 0.1) == RTMI_E_ARG and "noise" in err()
            for e in (-1.0, float("nan"), float("inf"), -float("inf")):
                assert call(ctx, nx, ny, ok, e) == RTMI_E_ARG and "eps" in err(), e
            for a, b in ((0, ny), (nx, 0), (-1, ny)):
                assert call(ctx, a, b, ok, 0.1) == RTMI_E_ARG, (a, b)
            for a, b in ((nx + 8, ny), (nx, ny - 1), (ny, nx)):  # not the frame's size
                assert call(ctx, a, b, ok, 0.1) == RTMI_E_STATE and ("%d x %d" % (a, b)) in err() and ("%d x %d" % (nx, ny)) in err(), (a, b)
        assert _retire(ctx, nx + 8, ny, ok, 0.1, n) == RTMI_E_STATE and n.value == -7
        assert ctx.adaptive_status() == status and ctx.progressive_samples() == k and np.array_equal(ctx.adaptive_active_tiles(), tiles)

    ft = cover.render_features(nx, ny, core.FEATURE_SAMPLES)[0]
    again = []
    for k0 in (0, 4, 8):
        lin, q, e, spp, cnt = cover.render_adaptive(nx, ny, k0, 4, 0.0)
        disturb()
        flt, fq, ferr = ctx.denoise(lin, e, ft)
        disturb()
        ctx.adaptive_retire(ferr, eps)
        disturb()
        again.append((k0 + 4, lin, q, e, spp, cnt, ctx.adaptive_status()[0], flt, fq, ferr))
    assert len(base) == 3 and all(a[0] == b[0] and a[6] == b[6] and _same(a[1:6], b[1:6]) and _same(a[7:], b[7:]) for a, b in zip(base, again))
    # no frame
    ctx.progressive_release()
    for call in (_retire, _retire_device):
        assert call(ctx, nx, ny, ok, 0.1) == RTMI_E_STATE and "no progressive frame" in err()
    assert ctx.adaptive_status() == (0, 0, 0)
    fresh = core.Context(0)
    try:
        assert _retire(fresh, nx, ny, ok, 0.1) == RTMI_E_STATE and fresh.adaptive_status() == (0, 0, 0)
    finally:
        fresh.close()


def test_progressive_continuation_and_frames_started_by_render_progressive(ctx, cover):
    L = r._ffi.lib()
    nx, ny = 200, 100
    tx, ty = fr.tiles_of(nx, ny)
    total = tx * ty
    bad, half = np.full((ny, nx), np.inf), np.zeros((ny, nx))
    half[:, : nx // 2] = np.inf  # the left tiles stay active (the middle column of tiles, cut by nx / 2 = 100 = 12.5 tiles, too)
    keep = ar.tile_max(half) > 0.5
    assert 0 < keep.sum() < total
    other = core.DeviceScene(r.scene.make_random_scene(96, 40, 3, False), ctx=ctx)
    try:
        # a retire that retired nothing leaves a uniform frame: render_progressive may continue it
        for start in ("adaptive", "progressive"):
            if start == "adaptive":
                cover.render_adaptive(nx, ny, 0, 4, 0.0)
            else:
                cover.render_progressive(nx, ny, 0, 4)
            other.render(96, 40, 2)  # rewrites the context's tile list: the conversion of a uniform frame must not read it as it stands
            assert ctx.adaptive_retire(bad, 0.5) == 0
            assert ctx.adaptive_status() == (total, total, nx * ny * 4) and np.array_equal(ctx.adaptive_active_tiles(), np.arange(total))
            lin, q, e, cnt = cover.render_progressive(nx, ny, 4, 3)
            assert _same((lin, q, cnt), cover.render(nx, ny, 7)), start
            assert ctx.adaptive_status() == (total, total, nx * ny * 7)
        # a frame started by render_progressive, some tiles retired: the frame a render_adaptive start gives, and render_progressive is refused
        ref = cover.render_adaptive(nx, ny, 0, 4, 0.0)
        assert ctx.adaptive_status()[0] == total, "nothing retires on the raw rule at eps 0 here: the input this test needs"
        assert ctx.adaptive_retire(half, 0.5) == total - keep.sum()
        ref2 = cover.render_adaptive(nx, ny, 4, 4, 0.0)
        ref_status = ctx.adaptive_status()
        lin, q, e, cnt = cover.render_progressive(nx, ny, 0, 4)
        assert _same((lin, q, e, cnt), (ref[0], ref[1], ref[2], ref[4]))
        other.render(96, 40, 2)
        assert ctx.adaptive_retire(half, 0.5) == total - keep.sum()
        assert np.array_equal(ctx.adaptive_active_tiles(), np.flatnonzero(keep.ravel()))
        status = ctx.adaptive_status()
        assert status == (int(keep.sum()), total, nx * ny * 4)
        rc = L.rtmi_render_progressive(cover.handle, nx, ny, 4, 4, 50, core.RENDER_SEED, 0, 0, 0, nx, ny, None, None, None, None)
        assert rc == RTMI_E_STATE and "retired" in L.rtmi_last_error().decode()
        rc = L.rtmi_render_progressive_device(cover.handle, nx, ny, 4, 4, 50, core.RENDER_SEED, 0, None, None, None, None, None)
        assert rc == RTMI_E_STATE and "retired" in L.rtmi_last_error().decode()
        assert ctx.adaptive_status() == status and ctx.progressive_samples() == 4
        got2 = cover.render_adaptive(nx, ny, 4, 4, 0.0)
        assert _same(got2, ref2) and ctx.adaptive_status() == ref_status
        assert np.array_equal(got2[3], ar.per_pixel(np.where(keep, 8, 4), nx, ny))
    finally:
        other.close()
        ctx.progressive_release()


# ---- 6. device form ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [False, True], ids=["caller's stream", "context's stream"])
def test_device_form_matches_host_form(ctx, cover, own_stream):
    import torch
    nx, ny, na = 200, 100, core.FEATURE_SAMPLES
    eps = _eps_from_first_round(cover, nx, ny, 4)
    host = list(cover.refine_adaptive_denoised(nx, ny, 12, 4, eps))
    lists = []
    ctx.progressive_release()
    st = torch.cuda.Stream()
    s = None if own_stream else st.cuda_stream
    with torch.cuda.stream(st):
        lin, flin = (torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda") for _ in range(2))
        q, fq = (torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        err, ferr = (torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(2))
        spp = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        ft = torch.zeros((ny, nx, 8), dtype=torch.float64, device="cuda")
        clean = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")  # a map on which every tile passes
    torch.cuda.synchronize()
    cover.render_features_device(nx, ny, na, ft, None, stream=s)
    assert len(host) == 3 and 0 < host[0][6] < 325  # tiles retire in the first round and tiles remain
    for k0, h in zip((0, 4, 8), host):
        # one stream, no host copy between the three calls: the filter reads what the render wrote, the retirement what the filter wrote
        cover.render_adaptive_device(nx, ny, k0, 4, 0.0, lin, q, err, spp, cnt, stream=s)
        before = ctx.adaptive_status()[0]
        ctx.denoise_device(nx, ny, lin, err, ft, flin, fq, ferr, stream=s)
        retired = ctx.adaptive_retire_device(nx, ny, ferr, eps, stream=s)  # synchronises the stream
        active = ctx.adaptive_status()[0]
        assert retired == before - active and active == h[6], (k0, retired, before, active)
        got = (lin.cpu().numpy(), q.cpu().numpy(), err.cpu().numpy(), spp.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64))
        assert _same(got, h[1:6]), k0
        assert _same((flin.cpu().numpy(), fq.cpu().numpy(), ferr.cpu().numpy()), h[7:]), k0
        lists.append(ctx.adaptive_active_tiles())
    assert ctx.adaptive_retire_device(nx, ny, clean, 0.0, stream=s) == len(lists[-1])
    assert ctx.adaptive_status()[0] == 0 and ctx.adaptive_retire_device(nx, ny, ferr, eps, stream=s) == 0
    ctx.progressive_release()


# ---- 7. interleaving -----------------------------------------------------------------------------------------------------------------------------------
def test_interleaved_calls_and_sample_passes(ctx, cover):
    nx, ny = 200, 100
    eps = _eps_from_first_round(cover, nx, ny, 4)
    base = list(cover.refine_adaptive_denoised(nx, ny, 16, 4, eps))
    assert len(np.unique(base[-1][4])) >= 2 and 0 < base[0][6] < ctx.adaptive_status()[1]
    ctx.set_option("workspace_bytes", 1 << 20)  # several sample passes per round
    try:
        small = list(cover.refine_adaptive_denoised(nx, ny, 16, 4, eps))
    finally:
        ctx.set_option("workspace_bytes", 8 << 30)
    assert len(base) == len(small) and all(_same(a[1:], b[1:]) for a, b in zip(base, small))
    other = core.DeviceScene(r.scene.make_random_scene(96, 40, 3, False), ctx=ctx)
    noise = dr.synthetic_frame(96, 40, seed=1)

    def between(i):
        other.render(96, 40, 3)  # another size on the same context rewrites the context's tile list, not the frame's
        other.render_features(96, 40, 2)
        ctx.denoise(*noise, iterations=2)  # another size through the denoise workspace and the staging buffer the host forms share
        ctx.set_option("accel", i % 2)

    ft = cover.render_features(nx, ny, core.FEATURE_SAMPLES)[0]
    mixed = []
    try:
        for i, k0 in enumerate((0, 4, 8, 12)):
            lin, q, e, spp, cnt = cover.render_adaptive(nx, ny, k0, 4, 0.0)
            between(i)
            flt, fq, ferr = ctx.denoise(lin, e, ft)
            between(i + 1)
            ctx.adaptive_retire(ferr, eps)
            between(i)
            mixed.append((k0 + 4, lin, q, e, spp, cnt, ctx.adaptive_status()[0], flt, fq, ferr))
    finally:
        ctx.set_option("accel", 1)
        other.close()
        ctx.progressive_release()
    assert len(base) == len(mixed) and all(a[6] == b[6] and _same(a[1:6], b[1:6]) and _same(a[7:], b[7:]) for a, b in zip(base, mixed))


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------------------------------------------
def _ppm(path, nx, ny):
    head = b"P6\n%d %d\n255\n" % (nx, ny)
    data = path.read_bytes()
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(ny, nx, 3)


def test_cli_adaptive_denoised(tmp_path, capsys):
    nx, ny = 64, 32
    out, flt = tmp_path / "a.ppm", tmp_path / "a.denoised.ppm"
    ds = core.DeviceScene(r.scene.make_random_scene(nx, ny, 11, True))
    try:
        eps = _eps_from_first_round(ds, nx, ny, 16)
        got = list(ds.refine_adaptive_denoised(nx, ny, 64, 16, eps))
        status = ds.ctx.adaptive_status()
        assert len(np.unique(got[-1][4])) >= 2
        assert core.main([str(out), "64", "32", "64", "--adaptive-denoised", repr(eps)]) == 0  # rounds of 16 by default, --denoise implied
        text = capsys.readouterr().out
        assert np.array_equal(_ppm(out, nx, ny), got[-1][2]) and np.array_equal(_ppm(flt, nx, ny), got[-1][8])
        assert not np.array_equal(got[-1][2], got[-1][8])
        assert ("samples: mean %.2f of 64 per pixel, %d of 32 tiles converged" % (status[2] / (nx * ny), 32 - status[0])) in text
        assert ("total-rays %d total-pixels %d" % (int(got[-1][5][0]), nx * ny)) in text
        assert ("wrote %s" % out) in text and ("wrote %s" % flt) in text
        # passes, feature samples and rounds as given
        ds.ctx.progressive_release()
        got = list(ds.refine_adaptive_denoised(nx, ny, 20, 8, eps, na=2, iterations=3))
        assert core.main([str(out), "64", "32", "20", "--adaptive-denoised=%r" % eps, "--chunk", "8", "--denoise", "3", "--feature-samples", "2"]) == 0
        text = capsys.readouterr().out
        assert np.array_equal(_ppm(out, nx, ny), got[-1][2]) and np.array_equal(_ppm(flt, nx, ny), got[-1][8])
        assert [g[0] for g in got][:3] == [8, 16, 20][:len(got)]
    finally:
        ds.ctx.progressive_release()
        ds.close()


# ---- 9. it must pay --------------------------------------------------------------------------------------------------------------------------------------
def test_it_pays_on_the_cornell_box(ctx):
    """Cornell box 128 x 128, first 16, chunk 16, cap 64, eps from the first round's filtered noise plane.  Asserted: the loop takes fewer
    pixel-samples than the uniform run to the cap, and its final filtered frame is closer (RMS) to a 4096-spp one-shot render of another seed
    than the 16-spp uniform frame filtered by the existing path -- the frame the loop starts from.  The rest is printed."""
    nx = ny = 128
    first, chunk, cap = 16, 16, 64
    ds = core.DeviceScene(r.scene.make_cornell_box(nx, ny), ctx=ctx)
    try:
        truth, _, _ = ds.render(nx, ny, 4096, seed=core.RENDER_SEED + 1)
        eps = _eps_from_first_round(ds, nx, ny, first)
        got = list(ds.refine_adaptive_denoised(nx, ny, cap, chunk, eps, first=first))
        active, total, pixel_samples = ctx.adaptive_status()
        ctx.progressive_release()
        share = pixel_samples / (nx * ny * cap)
        mean_spp = pixel_samples / (nx * ny)
        e_loop = dr.rms(got[-1][7], truth)
        e16 = dr.rms(ds.render_denoised(nx, ny, first)[2][0], truth)
        e_cap = dr.rms(ds.render_denoised(nx, ny, cap)[2][0], truth)
        e_same = dr.rms(ds.render_denoised(nx, ny, int(round(mean_spp)))[2][0], truth)
        print("cornell 128x128 eps %.5f: %.1f %% of the uniform run's pixel-samples (mean %.1f spp), %d of %d tiles still active at the cap; "
              "RMS error of the filtered frame: loop %.5f, uniform 16 spp %.5f, uniform %d spp %.5f, uniform %d spp (the cap) %.5f" % (
                  eps, 100 * share, mean_spp, active, total, e_loop, e16, int(round(mean_spp)), e_same, cap, e_cap))
        assert pixel_samples < nx * ny * cap
        assert e_loop < e16
    finally:
        ctx.progressive_release()
        ds.close()
