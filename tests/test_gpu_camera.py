"""The camera of a live scene on the device (rtmi_scene_set_camera, rtmi_scene_set_camera_stream, rtmi_scene_camera).  Every comparison is
np.array_equal of linear frame, 8-bit frame and counters between the LIVE scene after set_camera and a scene created FRESH from the same
arrays with that camera.  The live scene's tree was built for another camera: these are the first full renders through the traversal's
far-origin planes (a camera beyond the tree's bound), through a camera-ray stash whose width changes on a live scene (fixed origin <-> lens),
and through swept MovingSphere bounds that are wider than the camera's shutter."""
import copy
import ctypes as C

import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi, core, dist
from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import flatten as fl
from test_gpu_parity import RMS_TOL, rms

pytestmark = pytest.mark.gpu

NX, NY, NS = 60, 36, 4  # partial 8x8 tiles both ways
ASPECT = float(np.float32(NX)) / float(np.float32(NY))
RTMI_E_UNSUPPORTED, RTMI_E_STATE = -3, -5


def _lens(lookfrom, lookat=(0.0, 0.5, 0.0), aperture=0.3, t0=0.0, t1=1.0, vfov=20.0, aspect=ASPECT, focus_dist=10.0):
    return cam.thin_lens_camera(lookfrom=lookfrom, lookat=lookat, vup=[0.0, 1.0, 0.0], vfov=vfov, aspect=aspect, aperture=aperture,
                                focus_dist=focus_dist, t0=t0, t1=t1)


LENS = _lens([-6.0, 3.0, 8.0])                      # cam_fixed_origin 0: the stash is 17 words wide
LENS_CLOSED = _lens([-6.0, 3.0, 8.0], aperture=0.0)  # back to a fixed origin: 11 words
PINHOLE = cam.pinhole_camera(lookfrom=[3.0, 4.0, -10.0], lookat=[0.0, 0.5, 0.0], vup=[0.0, 1.0, 0.0], vfov=25.0, aspect=ASPECT)
NEG_ZERO = _lens([-0.0, 2.0, 12.0], aperture=0.0)    # origin + (+0) = +0 is not the origin bit for bit: no fixed origin although the lens is closed
# the ground sphere (radius 1000 about (0, -1000, 0)) puts the tree's bound at about 2002: every camera ray from here starts beyond it
FAR = _lens([5000.0, 800.0, 3000.0], lookat=(0.0, 0.0, 0.0), aperture=0.0, vfov=2.0, focus_dist=5900.0)


def _with_camera(flat, camera):
    f = copy.copy(flat)
    f.cam_kind, f.cam = fl.flatten_camera(camera)
    return f


def _fresh(flat, camera, ctx, render):
    """render(ds) of a scene created fresh from `flat` with `camera`"""
    ds = core.DeviceScene(_with_camera(flat, camera), ctx=ctx)
    try:
        return render(ds)
    finally:
        ds.close()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _bytes(ds):
    n = C.c_int64()
    core.check(_ffi.lib().rtmi_scene_device_bytes(ds.handle, C.byref(n)))
    return n.value


def _frame(nx=NX, ny=NY, ns=NS, precision="f64"):
    return lambda ds: ds.render(nx, ny, ns, precision=precision)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def static_scene():
    sc = r.scene.make_random_scene(NX, NY, 3, False)
    return fl.flatten(sc), sc["camera"]


@pytest.fixture(scope="module")
def moving_scene():
    sc = r.scene.make_random_scene(NX, NY, 11, True)
    return fl.flatten(sc), sc["camera"]  # its own camera: lookfrom (13, 2, 3), closed lens, shutter [0, 1]


# ---- 1. static spheres: a sequence of cameras on ONE live scene ------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 0], ids=["bvh", "flat"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_static_spheres_follow_a_sequence_of_cameras(ctx, static_scene, precision, accel):
    flat, own = static_scene
    ctx.set_option("accel", accel)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size = _bytes(live)
        info = live.camera_info()
        assert info["cam_kind"] == flat.cam_kind and info["cam"].tobytes() == np.ascontiguousarray(flat.cam, np.float64).tobytes()
        assert (info["built_t_lo"], info["built_t_hi"]) == (0.0, 1.0)
        for name, camera in (("own", own), ("lens", LENS), ("closed", LENS_CLOSED), ("pinhole", PINHOLE), ("-0", NEG_ZERO), ("far", FAR)):
            assert live.set_camera(camera) is False, name
            assert _bytes(live) == size, name
            kind, c24 = fl.flatten_camera(camera)
            info = live.camera_info()
            assert info["cam_kind"] == kind and info["cam"].tobytes() == c24.tobytes() and (info["built_t_lo"], info["built_t_hi"]) == (0.0, 1.0)
            got = _frame(precision=precision)(live)
            assert ctx.last_accel() == ("bvh" if accel else "flat")
            want = _fresh(flat, camera, ctx, _frame(precision=precision))
            assert _same(got, want), (name, precision, accel, float(np.abs(got[0] - want[0]).max()))
            assert got[2][1] == NX * NY and got[2][0] >= NX * NY * NS
    finally:
        live.close()
        ctx.set_option("accel", 1)


# ---- 2. moving spheres: the shutter decides between the fast path and the rebuild --------------------------------------------------------------
def test_moving_spheres_narrower_shutter_keeps_the_tree(ctx, moving_scene):
    flat, own = moving_scene
    narrow = _lens([13.0, 2.0, 3.0], lookat=(0.0, 0.0, 0.0), aperture=0.0, t0=0.25, t1=0.5)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size = _bytes(live)
        assert live.set_camera(narrow) is False and _bytes(live) == size
        info = live.camera_info()
        assert (info["built_t_lo"], info["built_t_hi"]) == (0.0, 1.0) and tuple(info["cam"][22:24]) == (0.25, 0.5)
        assert _same(_frame()(live), _fresh(flat, narrow, ctx, _frame()))
        swapped = _lens([-6.0, 3.0, 8.0], t0=0.75, t1=0.5)  # t0 > t1: the interval is [min, max]
        assert live.set_camera(swapped) is False
        assert _same(_frame()(live), _fresh(flat, swapped, ctx, _frame()))
    finally:
        live.close()


def test_moving_spheres_wider_shutter_rebuilds(ctx, moving_scene):
    flat, own = moving_scene
    narrow = _lens([13.0, 2.0, 3.0], lookat=(0.0, 0.0, 0.0), aperture=0.0, t0=0.25, t1=0.5)
    live = core.DeviceScene(_with_camera(flat, narrow), ctx=ctx)
    try:
        info = live.camera_info()
        assert (info["built_t_lo"], info["built_t_hi"]) == (0.25, 0.5)
        handle = live.handle.value
        assert live.set_camera(own) is True and live.handle.value == handle  # [0, 1] does not lie inside [0.25, 0.5]
        info = live.camera_info()
        assert (info["built_t_lo"], info["built_t_hi"]) == (0.0, 1.0) and tuple(info["cam"][22:24]) == (0.0, 1.0)
        assert _same(_frame()(live), _fresh(flat, own, ctx, _frame()))
        assert _same(_frame(precision="f32")(live), _fresh(flat, own, ctx, _frame(precision="f32")))
        # the rebuilt scene holds for [0, 1]: a pinhole camera (time 0) fits it now, and so does the narrow lens again
        assert live.set_camera(PINHOLE) is False and _same(_frame()(live), _fresh(flat, PINHOLE, ctx, _frame()))
        assert live.set_camera(narrow) is False and _same(_frame()(live), _fresh(flat, narrow, ctx, _frame()))
    finally:
        live.close()


def test_moving_spheres_pinhole_outside_the_built_shutter_rebuilds(ctx, moving_scene):
    """a scene whose bounds were built for [0.25, 0.5] is given a pinhole camera: its rays carry time 0, outside"""
    flat, own = moving_scene
    narrow = _lens([13.0, 2.0, 3.0], lookat=(0.0, 0.0, 0.0), aperture=0.0, t0=0.25, t1=0.5)
    live = core.DeviceScene(_with_camera(flat, narrow), ctx=ctx)
    try:
        assert live.set_camera(PINHOLE) is True
        info = live.camera_info()
        assert info["cam_kind"] == fl.CAM_PINHOLE and (info["built_t_lo"], info["built_t_hi"]) == (0.0, 0.0)
        assert _same(_frame()(live), _fresh(flat, PINHOLE, ctx, _frame()))
    finally:
        live.close()


def test_stream_form_refuses_a_shutter_that_does_not_fit(ctx, moving_scene):
    flat, own = moving_scene
    narrow = _lens([13.0, 2.0, 3.0], lookat=(0.0, 0.0, 0.0), aperture=0.0, t0=0.25, t1=0.5)
    live = core.DeviceScene(_with_camera(flat, narrow), ctx=ctx)
    try:
        before = _frame()(live)
        for camera in (own, PINHOLE):
            with pytest.raises(core.RtmiError) as e:
                live.set_camera(camera, stream=0)
            assert e.value.code == RTMI_E_UNSUPPORTED and "[0.25, 0.5]" in str(e.value), str(e.value)
        assert "[0, 0]" in str(e.value)  # both intervals are named: the pinhole's and the built one
        info = live.camera_info()
        assert tuple(info["cam"][22:24]) == (0.25, 0.5) and (info["built_t_lo"], info["built_t_hi"]) == (0.25, 0.5)
        assert _same(_frame()(live), before)
        inside = _lens([-6.0, 3.0, 8.0], t0=0.3, t1=0.45)  # one that fits travels on the stream
        assert live.set_camera(inside, stream=0) is False
        assert _same(_frame()(live), _fresh(flat, inside, ctx, _frame()))
    finally:
        live.close()


# ---- 3. mixed kinds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", ["0", "24"], ids=["tree", "small-scan"])
def test_cornell_box_follows_the_camera(ctx, monkeypatch, below):
    monkeypatch.setenv("RTMI_FLAT_BELOW", below)  # read per render: 24 answers the request for the tree with the small scan
    flat = fl.flatten(r.scene.make_cornell_box(48, 48))
    side = _lens([-300.0, 400.0, -700.0], lookat=(278.0, 278.0, 278.0), aperture=4.0, vfov=40.0, aspect=1.0, focus_dist=900.0)
    pin = cam.pinhole_camera(lookfrom=[278.0, 500.0, -760.0], lookat=[278.0, 200.0, 0.0], vup=[0.0, 1.0, 0.0], vfov=42.0, aspect=1.0)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size = _bytes(live)
        for camera in (side, pin):
            assert live.set_camera(camera) is False and _bytes(live) == size
            got = _frame(48, 48, 4)(live)
            assert ctx.last_accel() == ("flat" if below == "24" else "bvh")
            assert _same(got, _fresh(flat, camera, ctx, _frame(48, 48, 4)))
    finally:
        live.close()


def test_make_final_keeps_its_tables_through_a_rebuild(ctx):
    """a MovingSphere, two media, Perlin and image textures: the Perlin tables, the image and the media calls are not part of the rebuild and
    must have survived it"""
    sc = r.scene.make_final(64, 64)
    flat, own = fl.flatten(sc), sc["camera"]  # shutter [0, 1]
    half = _lens([478.0, 278.0, -600.0], lookat=(278.0, 278.0, 0.0), aperture=0.0, vfov=40.0, aspect=1.0, t0=0.0, t1=0.5)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size = _bytes(live)
        assert live.set_camera(half) is False and _bytes(live) == size  # narrower: the fast path
        assert live.camera_info()["built_t_hi"] == 1.0
        assert _same(_frame(64, 64, 2)(live), _fresh(flat, half, ctx, _frame(64, 64, 2)))
    finally:
        live.close()
    live = core.DeviceScene(_with_camera(flat, half), ctx=ctx)
    try:
        assert live.camera_info()["built_t_hi"] == 0.5
        assert live.set_camera(own) is True and live.camera_info()["built_t_hi"] == 1.0  # wider: the rebuild
        assert _same(_frame(64, 64, 2)(live), _fresh(flat, own, ctx, _frame(64, 64, 2)))
    finally:
        live.close()


# ---- 4. progressive and adaptive frames -------------------------------------------------------------------------------------------------------
def test_progressive_frame_is_not_continued_across_a_camera_move(ctx, static_scene):
    flat, own = static_scene
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        live.render_progressive(NX, NY, 0, 2)
        live.render_progressive(NX, NY, 2, 2)
        live.set_camera(LENS)
        with pytest.raises(core.RtmiError) as e:
            live.render_progressive(NX, NY, 4, 2)
        assert e.value.code == RTMI_E_STATE
        lin, q, err, cnt = live.render_progressive(NX, NY, 0, 4)
        assert _same((lin, q, cnt), _fresh(flat, LENS, ctx, _frame()))
        # the stream form changes the revision as well
        live.set_camera(PINHOLE, stream=0)
        with pytest.raises(core.RtmiError) as e:
            live.render_progressive(NX, NY, 4, 2)
        assert e.value.code == RTMI_E_STATE
        # ... and so does setting the very camera the scene already has: the bytes are not compared
        lin, q, err, cnt = live.render_progressive(NX, NY, 0, 2)
        live.set_camera(PINHOLE)
        with pytest.raises(core.RtmiError) as e:
            live.render_progressive(NX, NY, 2, 2)
        assert e.value.code == RTMI_E_STATE
    finally:
        ctx.progressive_release()
        live.close()


def test_adaptive_frame_is_not_continued_across_a_camera_move(ctx, static_scene):
    flat, own = static_scene
    eps = 0.05
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        live.render_adaptive(NX, NY, 0, 2, eps)
        live.render_adaptive(NX, NY, 2, 2, eps)
        live.set_camera(LENS)
        with pytest.raises(core.RtmiError) as e:
            live.render_adaptive(NX, NY, 4, 2, eps)
        assert e.value.code == RTMI_E_STATE
        got = live.render_adaptive(NX, NY, 0, 4, eps)
        active = ctx.adaptive_active_tiles()
        ctx.progressive_release()

        def fresh(ds):
            try:
                return ds.render_adaptive(NX, NY, 0, 4, eps), ctx.adaptive_active_tiles()
            finally:
                ctx.progressive_release()
        want, want_active = _fresh(flat, LENS, ctx, fresh)
        assert _same(got, want) and np.array_equal(active, want_active)
        assert _same((got[0], got[1], got[4]), _fresh(flat, LENS, ctx, _frame()))  # no tile retired before its 4 samples: the one-shot frame
    finally:
        ctx.progressive_release()
        live.close()


# ---- 5. features ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_features_follow_the_camera(ctx, static_scene, precision):
    flat, own = static_scene
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        for camera in (LENS, FAR):
            live.set_camera(camera)
            got = live.render_features(NX, NY, 2, precision=precision)
            assert _same(got, _fresh(flat, camera, ctx, lambda ds: ds.render_features(NX, NY, 2, precision=precision)))
            assert got[0][..., 7].max() == 1.0  # something was hit
    finally:
        live.close()


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------------------
def test_render_views_queues_cameras_and_frames_in_stream_order(ctx, static_scene):
    import torch
    flat, own = static_scene
    views = (own, LENS, FAR)  # fixed origin, lens, far origin
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        rgb8 = torch.zeros((3, NY, NX, 3), dtype=torch.uint8, device="cuda:%d" % ctx.device)
        out = live.render_views(views, NX, NY, NS, out_rgb8=rgb8)
        assert tuple(out.shape) == (3, NY, NX, 3) and out.dtype == torch.float64
        lin, q = out.cpu().numpy(), rgb8.cpu().numpy()
        for k, camera in enumerate(views):
            want = _fresh(flat, camera, ctx, _frame())
            assert np.array_equal(lin[k], want[0]) and np.array_equal(q[k], want[1]), k
        assert live.camera_info()["cam"].tobytes() == fl.flatten_camera(FAR)[1].tobytes()  # the scene keeps the last camera
    finally:
        live.close()


def test_a_render_queued_before_the_stream_form_keeps_the_old_camera(ctx, static_scene):
    import torch
    flat, own = static_scene
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        dev = "cuda:%d" % ctx.device
        a = torch.zeros((NY, NX, 3), dtype=torch.float64, device=dev)
        b = torch.zeros((NY, NX, 3), dtype=torch.float64, device=dev)
        ca = torch.zeros(2, dtype=torch.int64, device=dev)
        cb = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(ctx.device)
        live.render_device(NX, NY, NS, a, None, ca)   # old camera: fixed origin, 11-word stash
        live.set_camera(LENS, stream=0)               # no wait: the host mirror changes at once
        live.render_device(NX, NY, NS, b, None, cb)   # new camera: 17-word stash
        torch.cuda.synchronize(ctx.device)
        wa, wb = _fresh(flat, own, ctx, _frame()), _fresh(flat, LENS, ctx, _frame())
        assert np.array_equal(a.cpu().numpy(), wa[0]) and np.array_equal(ca.cpu().numpy().astype(np.uint64), wa[2])
        assert np.array_equal(b.cpu().numpy(), wb[0]) and np.array_equal(cb.cpu().numpy().astype(np.uint64), wb[2])
    finally:
        live.close()


# ---- 7. replicas ------------------------------------------------------------------------------------------------------------------------------
def test_replicas_and_clones_follow_the_camera(ctx, static_scene):
    flat, own = static_scene
    md = dist.MultiDevice(flat, [0, 0])
    try:
        assert md.set_camera(LENS) is False
        want = _fresh(flat, LENS, ctx, _frame())
        assert _same(md.render(NX, NY, NS), want)
        twin = md.scenes[1].clone(ctx)  # taken after set_camera: a clone replays the arguments the scene holds NOW
        try:
            assert twin.camera_info()["cam"].tobytes() == fl.flatten_camera(LENS)[1].tobytes()
            assert _same(_frame()(twin), want)
        finally:
            twin.close()
    finally:
        md.close()


def test_clone_of_a_rebuilt_scene(ctx, moving_scene):
    flat, own = moving_scene
    narrow = _lens([13.0, 2.0, 3.0], lookat=(0.0, 0.0, 0.0), aperture=0.0, t0=0.25, t1=0.5)
    live = core.DeviceScene(_with_camera(flat, narrow), ctx=ctx)
    try:
        assert live.set_camera(own) is True
        twin = live.clone(ctx)
        try:
            assert twin.camera_info()["built_t_hi"] == 1.0
            assert _same(_frame()(twin), _fresh(flat, own, ctx, _frame()))
        finally:
            twin.close()
    finally:
        live.close()


# ---- 8. one absolute pin ------------------------------------------------------------------------------------------------------------------------
def test_moved_camera_matches_the_oracle(ctx, static_scene, oracle):
    """the bound of test_render_matches_oracle (tests/test_gpu_parity.py), for the lens camera set on a scene built for another one"""
    flat, own = static_scene
    exp_lin, exp_q, exp_cnt = oracle.render(_with_camera(flat, LENS), NX, NY, NS, 50, core.RENDER_SEED, nthreads=16)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        live.set_camera(LENS)
        lin, q, cnt = live.render(NX, NY, NS)
    finally:
        live.close()
    assert rms(lin, exp_lin) <= RMS_TOL and rms(lin, exp_lin) < 1e-13
    assert np.array_equal(cnt, exp_cnt), "total-rays / total-pixels"
    assert np.abs(q.astype(int) - exp_q.astype(int)).max() <= 1 and (q != exp_q).mean() < 1e-3
