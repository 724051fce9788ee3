"""Occlusion rays generated on the device (rtmi_occlusion_hemisphere*, rtmi_occlusion_targets*, rtmi_ambient_occlusion*).  The rays the device builds
must equal the numpy restatement of include/rtmi.h (tests/occlusion_reference.py, camera.hemisphere_rays_disk) bit for bit; the flags, counts and
counters must equal what rtmi_query_occluded_device answers for those numpy rays, uploaded; the pixel-centre source must write rtmi_query_hits'
records of DeviceScene.pixel_centre_rays; and the whole pass must equal the numpy chain as exact doubles."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from raytrace_clj_amd import _ffi, camera, core
from tests import occlusion_reference as oref
from tests import visibility_cases as vc

FLT_MAX = vc.FLT_MAX
N_POINTS = 1500  # 23 1/2 waves of points
RANGES = ((0.001, FLT_MAX), (0.001, 1.0))
CASES = (("cover", "f64"), ("cover", "f32"), ("cornell", "f64"), ("layer(256)", "f64"), ("layer(256)", "f32"), ("mixed(65)", "f64"), ("hitlist-media", "f64"))
TARGETS = np.array([[0.0, 40.0, 0.0], [278.0, 554.0, 279.5], [13.0, 2.0, 3.0], [-4.0, 0.7, 9.0]])  # above the spheres, the Cornell lamp, the cover camera, low


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


@functools.lru_cache(maxsize=None)
def _open(name):
    """one context and device scene per recipe for the whole module"""
    ctx = core.Context(0)
    return ctx, core.DeviceScene(vc.flat(name), ctx=ctx)


def _dev():
    import torch
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _points(name):
    """(view rays [N_POINTS, 7], hit records on the host, the same in HBM, view rays in HBM): the first rays of the scene's set through
    query_hits_device, then records that yield no ray scattered over them (idle lanes in the middle of waves).  Computed once; do not write into them."""
    import torch
    ctx, ds = _open(name)
    view = np.ascontiguousarray(vc.rays(_oracle(), name)[:N_POINTS])
    d_view = torch.from_numpy(view).to(_dev())
    d_hits = torch.zeros((N_POINTS, _ffi.HIT_REC), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.query_hits_device(N_POINTS, d_view, d_hits)
    torch.cuda.synchronize(_dev())
    hits, touched = oref.degenerate(d_hits.cpu().numpy())
    assert (hits[:, 0] == 1).sum() > N_POINTS // 2
    d_hits = torch.from_numpy(hits).to(_dev())
    torch.cuda.synchronize(_dev())
    return view, hits, d_hits, d_view


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device_call(ds, kind, n, per, d_hits, d_view, precision, t_min, t_max, **kw):
    """one generated-source call on HBM buffers -> (rays, flags, counts, counters) on the host"""
    import torch
    m = n * per
    d_rays = torch.full((m, 7), -7.0, dtype=torch.float64, device=_dev())
    d_flags = torch.full((m,), 9, dtype=torch.uint8, device=_dev())
    d_counts = torch.full((n,), 9, dtype=torch.int32, device=_dev())
    d_cnt = torch.full((2,), 9, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize(_dev())
    out = dict(out_occluded=d_flags, out_count=d_counts, out_rays=d_rays, out_counters=d_cnt, precision=precision, t_min=t_min, t_max=t_max)
    if kind == "hemisphere":
        ds.occlusion_hemisphere_device(n, d_hits, per, view=d_view, **out, **kw)
    else:
        ds.occlusion_targets_device(n, d_hits, per, kw.pop("d_targets"), view=d_view, **out, **kw)
    torch.cuda.synchronize(_dev())
    return d_rays.cpu().numpy(), d_flags.cpu().numpy(), d_counts.cpu().numpy(), d_cnt.cpu().numpy().tolist()


def _expected_answers(ds, rays, ok, per, precision, t_min, t_max):
    """occluded_device on the numpy rays, uploaded, group = per; the rows of the points that yield no ray are left out of the call"""
    import torch
    rows = np.repeat(ok, per)
    flags = np.zeros(len(rays), np.uint8)
    some = np.ascontiguousarray(rays[rows])
    d_some = torch.from_numpy(some).to(_dev())
    d_flags = torch.zeros(len(some), dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.occluded_device(len(some) // per, per, d_some, out_occluded=d_flags, t_min=t_min, t_max=t_max, precision=precision)
    torch.cuda.synchronize(_dev())
    flags[rows] = d_flags.cpu().numpy()
    return flags, flags.reshape(-1, per).sum(axis=1).astype(np.int32), [int(rows.sum()), int(flags.sum())]


def _check(ds, name, what, got, exp_rays, ok, per, precision, ranges_done, rerun):
    rays, flags, counts, cnt = got
    assert rays.shape == exp_rays.shape
    diff = (_bits(rays) != _bits(exp_rays)).any(axis=1)
    assert not diff.any(), "%s: %d of %d rays differ from the restatement, first at row %d" % (what, diff.sum(), len(diff), int(np.flatnonzero(diff)[0]))
    for t_min, t_max in RANGES:
        if (t_min, t_max) != ranges_done:
            rays2, flags, counts, cnt = rerun(t_min, t_max)
            assert np.array_equal(_bits(rays2), _bits(exp_rays)), what
        e_flags, e_counts, e_cnt = _expected_answers(ds, exp_rays, ok, per, precision, t_min, t_max)
        where = "%s range (%g, %g)" % (what, t_min, t_max)
        assert flags.dtype == np.uint8 and np.array_equal(flags, e_flags), "%s: %d flags differ" % (where, (flags != e_flags).sum())
        assert np.array_equal(counts, e_counts), where + ": counts"
        assert cnt == e_cnt, (where, cnt, e_cnt)
    return e_flags


# ---- 1. the hemisphere source --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_hemisphere_rays_and_answers(name, precision):
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    some_occluded = some_free = False
    for n_dirs in (1, 5, 64, 70):       # 5 does not divide 64: runs straddle waves; 70: a group longer than a wave trip
        for first in (0, 3):
            for with_view in (True, False):
                v, dv = (view, d_view) if with_view else (None, None)
                exp_rays, ok = oref.hemisphere(hits, n_dirs, view=v, first=first, seed=77, time=0.25)
                assert 0 < ok.sum() < N_POINTS
                what = "%s %s n_dirs %d first %d view %s" % (name, precision, n_dirs, first, with_view)
                call = lambda t_min, t_max: _device_call(ds, "hemisphere", N_POINTS, n_dirs, d_hits, dv, precision, t_min, t_max, first=first, seed=77, time=0.25)  # noqa: E731
                e_flags = _check(ds, name, what, call(*RANGES[0]), exp_rays, ok, n_dirs, precision, RANGES[0], call)
                some_occluded |= bool(e_flags.any())
                some_free |= bool((e_flags[np.repeat(ok, n_dirs)] == 0).any())
    assert some_occluded and some_free, "the radius-1 flags of %s are all alike: nothing was compared" % name


@pytest.mark.parametrize("name", [n for n, p in CASES if p == "f64" and n not in vc.MEDIA_SCENES])
def test_hemisphere_flags_equal_the_oracles(name):
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    exp_rays, ok = oref.hemisphere(hits, 5, view=view, seed=77)
    rows = np.repeat(ok, 5)
    for t_min, t_max in RANGES:
        _, flags, _, _ = _device_call(ds, "hemisphere", N_POINTS, 5, d_hits, d_view, "f64", t_min, t_max, seed=77)
        orc = _oracle().probe_hit(vc.flat(name), np.ascontiguousarray(exp_rays[rows]), tmin=t_min, tmax=t_max)
        assert np.array_equal(flags[rows], orc[:, 0].astype(np.uint8)), (name, t_min, t_max)
        assert not flags[~rows].any()


# ---- 2. the targets source ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_targets_rays_and_answers(name, precision):
    import torch
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    for n_targets in (1, 4):
        tg = np.ascontiguousarray(TARGETS[:n_targets])
        d_tg = torch.from_numpy(tg).to(_dev())
        for with_view in (True, False):
            v, dv = (view, d_view) if with_view else (None, None)
            exp_rays, ok = oref.targets(hits, tg, view=v, time=0.5)
            assert ok.sum() > oref.yields_a_ray(hits).sum()  # (the zero normal and the infinite one send rays here)
            what = "%s %s targets %d view %s" % (name, precision, n_targets, with_view)
            call = lambda t_min, t_max: _device_call(ds, "targets", N_POINTS, n_targets, d_hits, dv, precision, t_min, t_max, d_targets=d_tg, time=0.5)  # noqa: E731
            _check(ds, name, what, call(*RANGES[0]), exp_rays, ok, n_targets, precision, RANGES[0], call)
    if name not in vc.MEDIA_SCENES and precision == "f64":
        rows = np.repeat(ok, 4)
        _, flags, _, _ = call(0.001, 1.0 - 0.001)  # "up to the target"
        orc = _oracle().probe_hit(vc.flat(name), np.ascontiguousarray(exp_rays[rows]), tmin=0.001, tmax=1.0 - 0.001)
        assert np.array_equal(flags[rows], orc[:, 0].astype(np.uint8))


# ---- 3. splits, host forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover", "cornell"))
def test_splits_over_first_and_the_host_forms(name):
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    f5, c5, n5, r5 = ds.occlusion_hemisphere(hits, 5, view=view, seed=9, t_max=1.0, return_rays=True)
    f3, c3, n3, r3 = ds.occlusion_hemisphere(hits, 3, view=view, first=0, seed=9, t_max=1.0, return_rays=True)
    f2, c2, n2, r2 = ds.occlusion_hemisphere(hits, 2, view=view, first=3, seed=9, t_max=1.0, return_rays=True)
    assert c5.any() and np.array_equal(c3 + c2, c5) and [int(a + b) for a, b in zip(n3, n2)] == [int(x) for x in n5]
    both = np.concatenate([r3.reshape(-1, 3, 7), r2.reshape(-1, 2, 7)], axis=1)
    assert np.array_equal(_bits(both), _bits(r5.reshape(-1, 5, 7)))
    assert np.array_equal(np.concatenate([f3.reshape(-1, 3), f2.reshape(-1, 2)], axis=1), f5.reshape(-1, 5))
    # the host forms run the device forms' launches
    rays, flags, counts, cnt = _device_call(ds, "hemisphere", N_POINTS, 5, d_hits, d_view, "f64", 0.001, 1.0, seed=9)
    assert np.array_equal(_bits(rays), _bits(r5)) and np.array_equal(flags, f5) and np.array_equal(counts, c5) and cnt == [int(x) for x in n5]
    tf, tc, tn, tr = ds.occlusion_targets(hits, TARGETS, view=view, return_rays=True)
    exp, ok = oref.targets(hits, TARGETS, view=view)
    assert np.array_equal(_bits(tr), _bits(exp)) and int(tn[0]) == 4 * int(ok.sum()) and np.array_equal(tc, tf.reshape(-1, 4).sum(axis=1))
    # every output is optional
    assert ds.occlusion_hemisphere(hits, 5, view=view, seed=9, t_max=1.0)[1].tolist() == c5.tolist()


# ---- 4. the pixel-centre source and the whole pass ------------------------------------------------------------------------------------------------
NX, NY = 40, 24


def _ao_buffers(nx, ny):
    import torch
    n = nx * ny
    return (torch.full((n,), -1.0, dtype=torch.float64, device=_dev()), torch.full((n,), 9, dtype=torch.int32, device=_dev()),
            torch.full((n, _ffi.HIT_REC), -1.0, dtype=torch.float64, device=_dev()), torch.zeros(2, dtype=torch.int64, device=_dev()))


def _ao_launch(ds, buf, nx, ny, n_dirs, radius, **kw):
    ds.ambient_occlusion_device(nx, ny, n_dirs, radius, out_visibility=buf[0], out_count=buf[1], out_hits=buf[2], out_counters=buf[3], **kw)


def _ao_read(buf, nx, ny):
    return buf[0].cpu().numpy().reshape(ny, nx), buf[1].cpu().numpy(), buf[2].cpu().numpy(), buf[3].cpu().numpy().tolist()


def _ao_device(ds, nx, ny, n_dirs, radius, **kw):
    import torch
    buf = _ao_buffers(nx, ny)
    torch.cuda.synchronize(_dev())
    _ao_launch(ds, buf, nx, ny, n_dirs, radius, **kw)
    torch.cuda.synchronize(_dev())
    return _ao_read(buf, nx, ny)


def _ao_chain(ds, nx, ny, n_dirs, radius, seed, first=0):
    """pixel_centre_rays -> query_hits -> occlusion_reference -> occluded, on the host"""
    primary = ds.pixel_centre_rays(nx, ny)
    hits = ds.query_hits(primary)
    rays, ok = oref.hemisphere(hits, n_dirs, view=primary, first=first, seed=seed)
    rows = np.repeat(ok, n_dirs)
    flags = np.zeros(len(rays), np.uint8)
    flags[rows] = ds.occluded(np.ascontiguousarray(rays[rows]), t_min=0.001, t_max=radius)[0]
    count = flags.reshape(-1, n_dirs).sum(axis=1).astype(np.int32)
    vis = 1.0 - count.astype(np.float64) / float(n_dirs)
    vis[hits[:, 0] == 0.0] = 1.0
    return vis.reshape(ny, nx), count, hits, [int(rows.sum()), int(flags.sum())]


@pytest.mark.parametrize("name", ("cover", "cornell"))
def test_pixel_centre_source_and_whole_pass(name):
    ctx = core.Context(0)
    ds = core.DeviceScene(vc.flat(name), ctx=ctx)
    try:
        kind = ds.camera_info()["cam_kind"]
        for moved in (False, True):
            if moved:
                # The camera travels in stream order.  Everything is allocated, filled and waited for BEFORE the move; then a call with the old
                # camera, the move and a call with the new camera are queued back to back on the context's stream with nothing between them,
                # and the host waits only afterwards.
                import torch
                c = np.asarray(ds.camera_info()["cam"], np.float64)
                rec = (camera.ThinLensCamera(c[0:3], c[3:6], c[6:9], c[9:12], c[12:15], c[15:18], c[18:21], c[21], c[22], c[23]) if kind != 0
                       else camera.PinholeCamera(c[0:3], c[3:6], c[6:9], c[9:12]))
                turned = camera.rotate_y(rec, 0.35, camera.view_pivot(rec))
                before, after = _ao_buffers(NX, NY), _ao_buffers(NX, NY)
                torch.cuda.synchronize(_dev())
                _ao_launch(ds, before, NX, NY, 6, 1.0, seed=31)
                ds.set_camera(turned, stream=0)
                _ao_launch(ds, after, NX, NY, 6, 1.0, seed=31)
                torch.cuda.synchronize(_dev())
                assert np.array_equal(_bits(_ao_read(before, NX, NY)[2]), _bits(first_hits)), "a call queued before the move saw the new camera"
                vis, count, hits, cnt = _ao_read(after, NX, NY)
            else:
                vis, count, hits, cnt = _ao_device(ds, NX, NY, 6, 1.0, seed=31)
            primary = ds.pixel_centre_rays(NX, NY)
            if kind != 0:
                assert (primary[:, 6] == ds.camera_info()["cam"][22]).all()
            e_vis, e_count, e_hits, e_cnt = _ao_chain(ds, NX, NY, 6, 1.0, 31)
            assert np.array_equal(_bits(hits), _bits(e_hits)), "%s moved %s: %d records differ" % (name, moved, (_bits(hits) != _bits(e_hits)).any(axis=1).sum())
            assert np.array_equal(count, e_count) and cnt == e_cnt
            assert np.array_equal(_bits(vis), _bits(e_vis))
            if name == "cornell":  # (nothing lies within 1.0 of a wall of the 555-unit box: a radius at which the blocks occlude)
                far = _ao_device(ds, NX, NY, 6, 150.0, seed=31)
                e_far = _ao_chain(ds, NX, NY, 6, 150.0, 31)
                assert np.array_equal(_bits(far[0]), _bits(e_far[0])) and np.array_equal(far[1], e_far[1]) and far[3] == e_far[3]
                vis, count = far[0], far[1]
            assert 0.0 < vis.mean() < 1.0
            if moved:
                assert not np.array_equal(hits, first_hits)
            first_hits = hits
        # the host form, the workspace in place of out_hits / out_count, and directions accumulated over calls
        radius = 150.0 if name == "cornell" else 1.0
        assert np.array_equal(ds.ambient_occlusion_device(NX, NY, 6, radius, seed=31), vis)
        c_a, c_b = np.zeros(NX * NY, np.int32), np.zeros(NX * NY, np.int32)
        ds.ambient_occlusion_device(NX, NY, 4, radius, seed=31, first=0, out_count=c_a)
        ds.ambient_occlusion_device(NX, NY, 2, radius, seed=31, first=4, out_count=c_b)
        assert np.array_equal(c_a + c_b, count)
    finally:
        ds.close()
        ctx.close()


def test_whole_pass_is_one_where_the_primary_ray_misses():
    ctx = core.Context(0)
    ds = core.DeviceScene(vc.count_flat(), ctx=ctx)  # layer(256, dome=False): the pixels above the horizon see nothing
    try:
        vis, count, hits, cnt = _ao_device(ds, NX, NY, 6, 1.0, seed=5)
        e_vis, e_count, e_hits, e_cnt = _ao_chain(ds, NX, NY, 6, 1.0, 5)
        miss = (e_hits[:, 0] == 0.0).reshape(NY, NX)
        assert miss.any() and (~miss).any()
        assert np.array_equal(_bits(hits), _bits(e_hits)) and np.array_equal(_bits(vis), _bits(e_vis)) and np.array_equal(count, e_count) and cnt == e_cnt
        assert (vis[miss] == 1.0).all() and (vis[~miss] < 1.0).any()
    finally:
        ds.close()
        ctx.close()


def _mean_and_variance(vis, n_dirs):
    v = vis.ravel()
    return float(v.mean()), float((v * (1.0 - v) / n_dirs).sum()) / float(len(v)) ** 2


def test_same_estimate_as_the_old_pass():
    """other directions, the same expectation: the image means differ by at most 5 sqrt(Va + Vb), V = sum v (1 - v) / 16 / N^2 (binomial).  The bound is
    checked for the oracle alone first (probe_hit on both generators' rays): if it did not hold there it would say nothing about the device."""
    nx, ny, n_dirs, radius = 64, 48, 16, 150.0  # (of a 555-unit box: the blocks and the corners occlude)
    ctx, ds = _open("cornell")
    f = vc.flat("cornell")
    primary = ds.pixel_centre_rays(nx, ny)
    h = _oracle().probe_hit(f, primary, tmin=0.001, tmax=FLT_MAX)
    hit = h[:, 0] == 1
    normals = h[:, 6:9].copy()
    away = (normals * primary[:, 3:6]).sum(axis=1) > 0.0
    normals[away] = -normals[away]
    images = []
    for gen in (camera.hemisphere_rays, camera.hemisphere_rays_disk):
        sec = gen(h[hit, 3:6], normals[hit], n_dirs, seed=core.RENDER_SEED, time=primary[0, 6])
        occ = _oracle().probe_hit(f, sec, tmin=0.001, tmax=radius)[:, 0].reshape(-1, n_dirs).sum(axis=1)
        vis = np.ones(nx * ny)
        vis[hit] = 1.0 - occ / float(n_dirs)
        images.append(vis)
    (ma, va), (mb, vb) = (_mean_and_variance(v, n_dirs) for v in images)
    print("oracle: means %.5f %.5f, bound %.5f" % (ma, mb, 5.0 * np.sqrt(va + vb)))
    assert abs(ma - mb) <= 5.0 * np.sqrt(va + vb), "the bound does not hold for the reference alone"
    old = ds.ambient_occlusion(nx, ny, n_dirs, radius)
    new = ds.ambient_occlusion_device(nx, ny, n_dirs, radius)
    assert old.shape == new.shape == (ny, nx) and not np.array_equal(old, new)
    (ma, va), (mb, vb) = _mean_and_variance(old, n_dirs), _mean_and_variance(new, n_dirs)
    print("device: means %.5f %.5f, bound %.5f" % (ma, mb, 5.0 * np.sqrt(va + vb)))
    assert abs(ma - mb) <= 5.0 * np.sqrt(va + vb)


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------------------
def _idle(ctx):
    import ctypes
    idle = ctypes.c_int32(-1)
    _ffi.check(_ffi.lib().rtmi_stream_idle(ctx.handle, ctypes.byref(idle)))
    return idle.value


def test_argument_errors_launch_nothing():
    ctx, ds = _open("cornell")
    view, hits, d_hits, d_view = _points("cornell")
    import torch
    torch.cuda.synchronize(_dev())
    assert _idle(ctx) == 1
    calls = (
        (lambda: ds.occlusion_hemisphere(hits, 0), -1),                                      # n_dirs = 0
        (lambda: ds.occlusion_hemisphere(hits, 4, first=-1), -1),                            # first < 0
        (lambda: ds.ambient_occlusion_device(NX, NY, 4, 0.0), -1),                           # radius <= 0
        (lambda: ds.ambient_occlusion_device(NX, NY, 4, -2.0), -1),
        (lambda: ds.ambient_occlusion_device(NX, NY, 0, 1.0), -1),
        (lambda: ds.occlusion_hemisphere_device(N_POINTS, None, 4), -1),                     # NULL hits
        (lambda: ds.occlusion_targets_device(N_POINTS, d_hits, 2, None), -1),                # NULL targets
        (lambda: ds.occlusion_hemisphere_device(2 ** 30, d_hits, 4), -1),                    # a product beyond 2^31 - 64
        (lambda: ds.occlusion_targets_device(2 ** 30, d_hits, 4, d_view), -1),
        (lambda: ds.ambient_occlusion_device(2 ** 15, 2 ** 15, 4, 1.0, out_visibility=d_view), -1),
        (lambda: ds.occlusion_hemisphere(hits, 4, precision="f32"), -3),                     # RTMI_F32 on a mixed-kind scene
        (lambda: ds.occlusion_targets(hits, TARGETS, precision="f32"), -3),
        (lambda: ds.ambient_occlusion_device(NX, NY, 4, 1.0, precision="f32"), -3),
    )
    for call, code in calls:
        with pytest.raises(_ffi.RtmiError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert _idle(ctx) == 1
    assert "FP64 only" in str(e.value)


def test_no_points_is_ok():
    ctx, ds = _open("cover")
    flags, counts, cnt = ds.occlusion_hemisphere(np.zeros((0, _ffi.HIT_REC)), 4)
    assert len(flags) == 0 and len(counts) == 0 and list(cnt) == [0, 0]
    flags, counts, cnt = ds.occlusion_targets(np.zeros((0, _ffi.HIT_REC)), TARGETS)
    assert len(flags) == 0 and len(counts) == 0 and list(cnt) == [0, 0]
    ds.occlusion_hemisphere_device(0, None, 4)
    ds.occlusion_targets_device(0, None, 2, None)
    assert ds.ambient_occlusion_device(0, NY, 4, 1.0).shape == (NY, 0)
