"""The geometry of a live scene on the device (rtmi_scene_set_geometry, refit_kernel).  Every comparison is np.array_equal of linear frame, 8-bit
frame and ray counter between the LIVE scene after set_geometry and a DeviceScene created FRESH from the edited FlatScene; where stated also of
rtmi_probe_hit on a few hundred rays and of the feature buffers.  All frames are 36x20 (partial 8x8 tiles on both edges), 4 samples, depth 50.
The node array the device refit is compared, byte for byte, with the host reference's (rtmi_test_refit), which test_geometry_host.py checks
against numpy."""
import copy
import ctypes as C

import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi, core, dist
from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import flatten as fl
import geometry_cases as gc

pytestmark = pytest.mark.gpu

NX, NY, NS = gc.NX, gc.NY, gc.NS
ASPECT = float(np.float32(NX)) / float(np.float32(NY))
RTMI_E_ARG, RTMI_E_STATE = -1, -5


def _fresh(flat, ctx, render):
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        return render(ds)
    finally:
        ds.close()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _frame(precision="f64"):
    return lambda ds: ds.render(NX, NY, NS, precision=precision)


def _with_camera(flat, camera):
    f = copy.copy(flat)
    f.cam_kind, f.cam = fl.flatten_camera(camera)
    return f


def _bytes(ds):
    n = C.c_int64()
    core.check(_ffi.lib().rtmi_scene_device_bytes(ds.handle, C.byref(n)))
    return n.value


def _nodes(ds):
    n = C.c_int64()
    core.check(_ffi.lib().rtmi_test_scene_nodes(ds.handle, None, 0, C.byref(n)))
    buf = np.zeros(max(n.value, 1), np.uint8)
    core.check(_ffi.lib().rtmi_test_scene_nodes(ds.handle, _ffi.ptr(buf), len(buf), C.byref(n)))
    return buf[:n.value]


def _rays(flat, n=300, seed=3):
    """rays from around the camera into the scene: origin, direction, time"""
    rng = np.random.default_rng(seed)
    o = np.asarray(flat.cam[0:3])[None, :] + rng.standard_normal((n, 3)) * 0.05
    d = -o / np.linalg.norm(o, axis=1)[:, None] + rng.standard_normal((n, 3)) * 0.3
    return np.concatenate([o, d, rng.random((n, 1))], axis=1)


def _agrees(live, edited, ctx, probes=True, features=False, precisions=("f64", "f32")):
    for precision in precisions:
        got, want = _frame(precision)(live), _fresh(edited, ctx, _frame(precision))
        assert _same(got, want), (precision, float(np.abs(got[0] - want[0]).max()))
        assert got[2][1] == NX * NY
        if probes:
            rays = _rays(edited)
            assert np.array_equal(live.probe_hit(rays, precision=precision), _fresh(edited, ctx, lambda ds: ds.probe_hit(rays, precision=precision)), equal_nan=True)
    if features:
        assert _same(live.render_features(NX, NY), _fresh(edited, ctx, lambda ds: ds.render_features(NX, NY)))


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cover():
    return gc.cover()


@pytest.fixture(scope="module")
def cover_frame(cover, ctx):
    return _fresh(cover, ctx, _frame())


def _carry(A, which, lift=1.0):
    def change(q, xp):
        for i in which:
            q[i, 0], q[i, 2] = -q[i, 0] * 0.5, -q[i, 2] * 0.5
            q[i, 1] += lift
    return gc.edited(A, change)


# ---- 1. the grid scene ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 0])
def test_grid_scene_refit_only(ctx, cover, cover_frame, accel):
    """several radii shrunk and centres moved by 1e-3: nothing is displaced, the whole node array is refit, and it is the host reference's"""
    B = gc.shrink_and_nudge(cover, gc.small_spheres(cover)[::3])
    live = core.DeviceScene(cover, ctx=ctx)
    try:
        tree = live.tree_info()
        assert tree[2] > 0  # an entry grid was built
        before = _bytes(live)
        info = live.set_geometry(B)
        assert (info["rebuilt"], info["displaced"]) == (False, 0) and info["nodes_refit"] > 0 and info["launches"] >= 1
        assert live.flat is not cover and np.array_equal(live.flat.prim_geom, B.prim_geom)
        ref = gc.refit([cover, B])
        assert (ref["rebuilt"], ref["records"], ref["launches"]) == (0, info["nodes_refit"], info["launches"]) and ref["grid_n"] > 0
        assert np.array_equal(_nodes(live), ref["nodes"])  # refit_kernel against the host's reference, bit for bit
        ctx.set_option("accel", accel)
        try:
            _agrees(live, B, ctx, features=accel == 1)
            assert not _same(_frame()(live)[:2], cover_frame[:2])  # the edit is visible
        finally:
            ctx.set_option("accel", 1)
        assert live.tree_info() == tree
        after = _bytes(live)
        assert after > before  # the refit plan and the leaf boxes are counted ...
        live.set_geometry(cover)
        assert _bytes(live) == after  # ... once: nothing is allocated after the first edit
        assert np.array_equal(_nodes(live), gc.refit([cover])["nodes"])  # back where it was built: the builder's own array
        assert _same(_frame()(live), cover_frame)
    finally:
        live.close()


def test_grid_scene_one_displaced(ctx, cover):
    small = gc.small_spheres(cover)
    i = int(small[len(small) // 2])
    B = _carry(cover, [i])
    C2 = gc.edited(B, lambda q, xp: q.__setitem__((i, 0), q[i, 0] + 0.75))
    live = core.DeviceScene(cover, ctx=ctx)
    try:
        n_big = live.tree_info()[3]
        info = live.set_geometry(B)  # carried across the layer and lifted above it
        assert (info["rebuilt"], info["displaced"]) == (False, 1)
        ref = gc.refit([cover, B])
        assert ref["displaced"] == 1 and i in ref["big"] and np.array_equal(_nodes(live), ref["nodes"])
        assert live.tree_info()[3] == n_big + 1  # the big list is one longer
        _agrees(live, B, ctx, features=True)
        info = live.set_geometry(C2)  # moved again: still the one displaced primitive
        assert (info["rebuilt"], info["displaced"]) == (False, 1)
        assert np.array_equal(_nodes(live), gc.refit([cover, B, C2])["nodes"])
        _agrees(live, C2, ctx)
        info = live.set_geometry(C2, mode="rebuild")  # a fresh tree brings it home
        assert (info["rebuilt"], info["displaced"], info["nodes_refit"]) == (True, 0, 0)
        assert np.array_equal(_nodes(live), gc.refit([C2])["nodes"])
        _agrees(live, C2, ctx)
        assert live.tree_info()[3] == n_big
    finally:
        live.close()


def test_grid_scene_rebuild_paths(ctx, cover):
    small = gc.small_spheres(cover)
    live = core.DeviceScene(cover, ctx=ctx)
    try:
        room = 16 - gc.refit([cover], want_nodes=False)["n_big"]
        full = _carry(cover, small[:room])
        info = live.set_geometry(full)  # the big list filled to its sixteen entries: still in place
        assert (info["rebuilt"], info["displaced"]) == (False, room)
        _agrees(live, full, ctx, precisions=("f64",))
        over = _carry(cover, small[:room + 1])
        info = live.set_geometry(over)  # one more overflows it
        assert (info["rebuilt"], info["displaced"]) == (True, 0)
        _agrees(live, over, ctx, precisions=("f64",))
        far = gc.edited(cover, lambda q, xp: q.__setitem__((int(small[0]), 0), 5000.0))  # beyond the bound the trees were built for
        info = live.set_geometry(far)
        assert (info["rebuilt"], info["displaced"]) == (True, 0)
        _agrees(live, far, ctx, precisions=("f64",))
    finally:
        live.close()


def test_big_primitives(ctx, cover):
    """the ground's radius and centre: a big primitive, in no tree"""
    ground = int(np.argmax(np.abs(cover.prim_geom[:, 3]) * (np.asarray(cover.prim_geom[:, 1]) < 0)))

    def change(q, xp):
        q[ground, 3] -= 0.05
        q[ground, 1] += 0.02
        q[ground, 0] += 0.5
    B = gc.edited(cover, change)
    live = core.DeviceScene(cover, ctx=ctx)
    try:
        info = live.set_geometry(B)
        assert (info["rebuilt"], info["displaced"]) == (False, 0)
        assert np.array_equal(_nodes(live), gc.refit([cover])["nodes"])  # the refit ran and changed nothing: no leaf moved
        _agrees(live, B, ctx, features=True)
    finally:
        live.close()


# ---- 2. the mixed-kind kernels ------------------------------------------------------------------------------------------------------------------
def _cornell_edit(flat):
    """the tall block's Translate offset and RotateY (sin, cos), the lamp moved, a wall pushed back"""
    tr = np.flatnonzero(flat.xform_kind == fl.XFORM_TRANSLATE)
    ro = np.flatnonzero(flat.xform_kind == fl.XFORM_ROTATE_Y)
    k = gc.kinds(flat)

    def change(g, xp):
        xp[tr[-1], 0] += 17.0
        xp[tr[-1], 2] -= 23.0
        a = np.arctan2(xp[ro[-1], 0], xp[ro[-1], 1]) + 0.2
        xp[ro[-1], 0], xp[ro[-1], 1] = np.sin(a), np.cos(a)
        lamp = int(np.flatnonzero(k == fl.PRIM_RECT_XZ)[0])
        g[lamp, 0] -= 40.0
        g[lamp, 2] -= 40.0
        wall = int(np.flatnonzero(k == fl.PRIM_RECT_XY)[0])
        g[wall, 4] -= 6.0
    return gc.edited(flat, change)


@pytest.mark.parametrize("path", ["small-scan", "tree", "flat"])
def test_cornell_box(ctx, monkeypatch, path):
    if path == "tree":
        monkeypatch.setenv("RTMI_SMALL_SCAN", "0")
    flat = fl.flatten(r.scene.make_cornell_box(NX, NY))
    B = _cornell_edit(flat)
    ctx.set_option("flat_below", 0)
    ctx.set_option("accel", 0 if path == "flat" else 1)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        info = live.set_geometry(B)
        assert (info["rebuilt"], info["displaced"]) == (False, 0)
        assert np.array_equal(_nodes(live), gc.refit([flat, B])["nodes"])
        assert not _same(_frame()(live)[:2], _fresh(flat, ctx, _frame())[:2])
        _agrees(live, B, ctx, features=path == "tree", precisions=("f64",))
    finally:
        ctx.set_option("flat_below", 24)
        ctx.set_option("accel", 1)
        live.close()


def test_a_triangles_vertex(ctx):
    flat = fl.flatten(r.scene.make_two_triangles(NX, NY))
    t = int(np.flatnonzero(gc.kinds(flat) == fl.PRIM_TRIANGLE)[0])
    B = gc.edited(flat, lambda g, xp: g.__setitem__((t, slice(0, 3)), g[t, 0:3] * 0.9))
    ctx.set_option("flat_below", 0)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        assert live.set_geometry(B)["rebuilt"] is False
        _agrees(live, B, ctx, precisions=("f64",))
    finally:
        ctx.set_option("flat_below", 24)
        live.close()


def test_media(ctx):
    """the smoke variant: a boundary primitive edited (a medium's fast operands follow, where it has them), and a medium row changed -> rebuilt"""
    H, S, T = r.hitable, r.shader, r.texture
    grey = S.lambertian(albedo=T.constant(color=np.array([0.6, 0.6, 0.6])))
    light = S.diffuse_light(tex=T.constant(color=np.array([2.0, 2.0, 2.0])))
    ball = H.constant_medium(boundary=H.sphere(center=np.array([0.0, 0.6, 0.0]), radius=0.6, material=grey), density=1.5, albedo=T.constant(color=np.ones(3)))
    items = [H.sphere(center=np.zeros(3), radius=40.0, material=light), H.sphere(center=np.array([0.0, -100.0, 0.0]), radius=100.0, material=grey), ball,
             H.sphere(center=np.array([1.4, 0.4, 0.3]), radius=0.4, material=grey)]
    camera = cam.pinhole_camera(lookfrom=np.array([5.0, 1.5, 2.0]), lookat=np.array([0.0, 0.5, 0.0]), vup=np.array([0.0, 1.0, 0.0]), vfov=30.0, aspect=ASPECT)
    scenes = [fl.flatten({"camera": camera, "world": H.hitlist(items=items)}), fl.flatten(r.scene.make_cornell_box(NX, NY, classic=False))]
    for flat in scenes:
        b = int(np.flatnonzero((np.asarray(flat.prim_kind) & fl.PRIM_BOUNDARY) != 0)[0])
        medium = int(np.flatnonzero(gc.kinds(flat) == fl.PRIM_MEDIUM)[0])
        sphere = gc.kinds(flat)[b] <= fl.PRIM_UVSPHERE
        B = gc.edited(flat, (lambda g, xp: g.__setitem__((b, slice(0, 4)), g[b, 0:4] * [1.0, 0.8, 1.0, 0.8])) if sphere else
                      (lambda g, xp: g.__setitem__((b, 4), g[b, 4] - 20.0)))
        live = core.DeviceScene(flat, ctx=ctx)
        try:
            assert live.set_geometry(B)["rebuilt"] is False
            assert not _same(_frame()(live)[:2], _fresh(flat, ctx, _frame())[:2])
            _agrees(live, B, ctx, precisions=("f64",))
            D = gc.edited(B, lambda g, xp: g.__setitem__((medium, 0), g[medium, 0] * 0.5))
            assert live.set_geometry(D)["rebuilt"] is True  # a medium's row is structure: the scene is rebuilt
            _agrees(live, D, ctx, precisions=("f64",))
        finally:
            live.close()


def test_moving_spheres_and_the_built_shutter(ctx):
    sc = r.scene.make_random_scene(NX, NY, 3, True)
    flat, own = fl.flatten(sc), sc["camera"]
    moving = np.flatnonzero(gc.kinds(flat) == fl.PRIM_MOVING)
    B = gc.edited(flat, lambda g, xp: g.__setitem__((moving, 5), g[moving, 5] * 0.5))  # center1: every sweep half as high
    narrow = cam.thin_lens_camera(lookfrom=[13.0, 2.0, 3.0], lookat=[0.0, 0.0, 0.0], vup=[0.0, 1.0, 0.0], vfov=20.0, aspect=ASPECT, aperture=0.0,
                                  focus_dist=10.0, t0=0.25, t1=0.5)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        assert live.set_geometry(B)["rebuilt"] is False
        assert np.array_equal(_nodes(live), gc.refit([flat, B])["nodes"])
        _agrees(live, B, ctx)
        assert live.set_camera(narrow) is False  # a shutter inside the built interval: the boxes swept over [0, 1] hold
        _agrees(live, _with_camera(B, narrow), ctx, probes=False)
        assert live.set_geometry(flat)["rebuilt"] is False  # ... and an edit under that camera is swept over the BUILT interval
        _agrees(live, _with_camera(flat, narrow), ctx, probes=False)
        assert live.set_camera(own) is False
        _agrees(live, flat, ctx, probes=False, precisions=("f64",))
    finally:
        live.close()


# ---- 3. sequences, and what replays the scene's arguments ---------------------------------------------------------------------------------------
def test_sequences(ctx, cover):
    small = gc.small_spheres(cover)
    B = gc.shrink_and_nudge(cover, small[::2])
    C3 = _carry(gc.shrink_and_nudge(B, small[1::2], factor=0.8), [int(small[7])])
    live = core.DeviceScene(cover, ctx=ctx)
    try:
        live.set_geometry(B)
        info = live.set_geometry(C3)
        assert (info["rebuilt"], info["displaced"]) == (False, 1)
        _agrees(live, C3, ctx, precisions=("f64",))
        # a material edit after a geometry edit
        M = copy.copy(C3)
        M.tex_param = np.array(C3.tex_param)
        M.tex_param[int(np.flatnonzero(C3.tex_kind == fl.TEX_CONSTANT)[0]), 0:3] = (0.9, 0.1, 0.2)
        assert live.set_materials(M) is False
        _agrees(live, M, ctx, probes=False, precisions=("f64",))
        # a clone replays the scene's arguments: the edited geometry, a fresh tree
        twin = live.clone(ctx)
        try:
            assert _same(_frame()(twin), _frame()(live))
            assert twin.set_geometry(cover)["displaced"] == 0 and np.array_equal(live.flat.prim_geom, C3.prim_geom)
        finally:
            twin.close()
        _agrees(live, M, ctx, probes=False, precisions=("f64",))
    finally:
        live.close()


def test_a_camera_rebuild_after_an_edit_keeps_it(ctx):
    sc = r.scene.make_random_scene(NX, NY, 3, True)
    flat, own = fl.flatten(sc), sc["camera"]
    narrow = cam.thin_lens_camera(lookfrom=[13.0, 2.0, 3.0], lookat=[0.0, 0.0, 0.0], vup=[0.0, 1.0, 0.0], vfov=20.0, aspect=ASPECT, aperture=0.0,
                                  focus_dist=10.0, t0=0.25, t1=0.5)
    B = gc.shrink_and_nudge(flat, gc.small_spheres(flat)[::2])
    live = core.DeviceScene(_with_camera(flat, narrow), ctx=ctx)
    try:
        assert live.set_geometry(B)["rebuilt"] is False
        _agrees(live, _with_camera(B, narrow), ctx, probes=False, precisions=("f64",))
        assert live.set_camera(own) is True  # the shutter [0, 1] does not fit the built [0.25, 0.5]: rebuilt from the arrays the scene holds NOW
        _agrees(live, _with_camera(B, own), ctx, probes=False, precisions=("f64",))
        assert live.set_geometry(flat)["rebuilt"] is False  # the plan of the old node array was dropped with it
        _agrees(live, _with_camera(flat, own), ctx, probes=False, precisions=("f64",))
    finally:
        live.close()


def test_progressive_and_adaptive_frames_restart(ctx, cover):
    B = gc.shrink_and_nudge(cover, gc.small_spheres(cover)[::3])
    live = core.DeviceScene(cover, ctx=ctx)
    try:
        for f, mode in ((B, "auto"), (B, "auto"), (cover, "rebuild")):  # the second sets what the scene already has: the revision moves all the same
            live.render_progressive(NX, NY, 0, 2)
            live.set_geometry(f, mode=mode)
            with pytest.raises(core.RtmiError) as e:
                live.render_progressive(NX, NY, 2, 2)
            assert e.value.code == RTMI_E_STATE
            with pytest.raises(core.RtmiError) as e:
                live.render_adaptive(NX, NY, 2, 2, 0.05)
            assert e.value.code == RTMI_E_STATE
            lin, q, err, cnt = live.render_progressive(NX, NY, 0, NS)
            assert _same((lin, q, cnt), _fresh(f, ctx, _frame()))
    finally:
        ctx.progressive_release()
        live.close()


def test_bad_input_leaves_the_scene_as_it_was(ctx):
    flat = fl.flatten(r.scene.make_cornell_box(NX, NY, classic=False))
    medium = int(np.flatnonzero(gc.kinds(flat) == fl.PRIM_MEDIUM)[0])
    bad = {
        "boundary range": gc.edited(flat, lambda g, xp: g.__setitem__((medium, 2), 1000.0)),
        "boundary range ": gc.edited(flat, lambda g, xp: g.__setitem__((medium, 1), -1.0)),
        "medium": gc.edited(flat, lambda g, xp: g.__setitem__((medium, 0), np.nan)),
    }
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size, before = _bytes(live), _frame()(live)
        live.render_progressive(NX, NY, 0, 2)
        for what, f in bad.items():
            with pytest.raises(core.RtmiError) as created:
                core.DeviceScene(f, ctx=ctx)
            for mode in ("auto", "rebuild"):
                with pytest.raises(core.RtmiError) as e:
                    live.set_geometry(f, mode=mode)
                assert e.value.code == created.value.code == RTMI_E_ARG and what.strip() in str(e.value), (what, str(e.value))
        # other counts than the scene's, straight at the C-ABI: a changed count is a new scene
        g = np.zeros((len(flat.prim_kind) + 1, fl.PRIM_STRIDE))
        assert _ffi.lib().rtmi_scene_set_geometry(live.handle, len(g), _ffi.ptr(g), len(flat.xform_kind), None, 0, None) == RTMI_E_ARG
        assert "new scene" in _ffi.lib().rtmi_last_error().decode()
        assert live.flat is flat and _bytes(live) == size
        live.render_progressive(NX, NY, 2, 2)  # not even the revision moved: the frame started before goes on
        ctx.progressive_release()
        assert _same(_frame()(live), before)
    finally:
        ctx.progressive_release()
        live.close()


# ---- 4. several hosts ---------------------------------------------------------------------------------------------------------------------------
def test_replicas_follow_an_edit(ctx, cover):
    B = _carry(gc.shrink_and_nudge(cover, gc.small_spheres(cover)[::3]), [int(gc.small_spheres(cover)[4])])
    md = dist.MultiDevice(cover, [0, 0])
    try:
        info = md.set_geometry(B)
        assert (info["rebuilt"], info["displaced"]) == (False, 1)
        assert _same(md.render(NX, NY, NS), _fresh(B, ctx, _frame()))
        with pytest.raises(ValueError):
            md.set_geometry(fl.flatten(r.scene.make_two_spheres(NX, NY)))
        assert all(np.array_equal(s.flat.prim_geom, B.prim_geom) for s in md.scenes)
        assert _same(md.render(NX, NY, NS), _fresh(B, ctx, _frame()))
    finally:
        md.close()


def test_the_accumulator_drops_its_history_at_an_edit(ctx):
    sc = r.scene.make_random_scene(NX, NY, 3, False)
    flat, own = fl.flatten(sc), sc["camera"]
    B = gc.shrink_and_nudge(flat, gc.small_spheres(flat), factor=0.7)
    views = cam.orbit(own, 120)[:3]
    seed = 77
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        acc = core.TemporalAccumulator(live, NX, NY, NS, seed=seed)
        assert acc.step(views[0])[4] == 0.0
        assert acc.step(views[1])[4] > 0.0
        lin, q, se, w, share = acc.step(views[2], geometry=B)
        assert share == 0.0 and (w.cpu().numpy() == NS).all()
        own_frame = _fresh(_with_camera(B, views[2]), ctx, lambda ds: ds.render_progressive(NX, NY, 0, NS, core.DEFAULT_DEPTH, seed + 2))
        assert np.array_equal(lin.cpu().numpy(), own_frame[0]) and np.array_equal(q.cpu().numpy(), own_frame[1])
        assert np.array_equal(se.cpu().numpy(), own_frame[2], equal_nan=True) and np.array_equal(acc.rays, own_frame[3])
        assert acc.step(views[1])[4] > 0.0  # the step after it takes history again
    finally:
        ctx.progressive_release()
        live.close()
