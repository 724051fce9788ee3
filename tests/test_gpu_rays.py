"""rtmi_render_rays*: caller-supplied rays through the tracer.

The yardstick is the device's own probe_paths -- pinned to the oracle segment for segment elsewhere -- and the frames the render entry points produce:
a ray traced here is the probe's path bit for bit, a group folded here is a pixel's samples folded by the frame (rays_reference.fold), and the pinhole
rays of a frame, grouped per pixel, give that frame.  Scenes and camera rays are depth_cases'; the refill test's input and its condition on the oracle
are rays_reference's (test_rays_reference.py holds the condition)."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import frame_reference as fr
import rays_reference as rr
import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi, core
from raytrace_clj_amd import camera as cam

pytestmark = pytest.mark.gpu

N = 3000                       # camera rays per scene: twelve workgroups of the probe, 47 waves, the last one partial
BIG_SEED = 0xFEDCBA9876543210  # high 32 bits set


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    """name or FlatScene -> DeviceScene on the module's context, made once"""
    made = {}

    def get(scene):
        key = scene if isinstance(scene, str) else id(scene)
        if key not in made:
            made[key] = core.DeviceScene(dc.flat(scene) if isinstance(scene, str) else scene, ctx=ctx)
        return made[key]

    yield get
    for ds in made.values():
        ds.close()


def _set(ctx, **options):
    for k, v in options.items():
        ctx.set_option(k, v)


def _equal(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. per ray ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 1, 50])
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("name", rr.SCENES)
def test_every_ray_is_the_probes_path(ctx, scenes, oracle, name, accel, depth):
    rays, keys, ctr0 = dc.camera_paths(oracle, name, N)
    ds = scenes(name)
    _set(ctx, accel=accel)
    try:
        mean, err, cnt, out = ds.render_rays(rays, 1, keys, ctr0=ctr0, depth=depth, return_rays=True)
        rgb, nseg, _, _ = ds.probe_paths(rays, keys, depth=depth, ctr0=ctr0)
    finally:
        _set(ctx, accel=1)
    assert np.array_equal(out, rgb), "%d rays differ from the probe's" % (out != rgb).any(axis=1).sum()
    assert int(cnt[0]) == int(nseg.sum()) and int(cnt[1]) == N
    assert np.array_equal(mean, out) and np.isposinf(err).all()       # a group of one: the ray itself, no noise estimate
    ergb, enseg, _, _ = oracle.probe_paths(dc.flat(name), rays, keys, depth=depth, ctr0=ctr0)
    if dc.SCENES[name][3]:
        assert np.array_equal(nseg, enseg)
        assert np.abs(out - ergb).max() <= 1e-11, np.abs(out - ergb).max()
    else:  # the media rule of depth_cases.check_paths
        same = nseg == enseg
        assert same.mean() > dc.MEDIA_SAME
        assert np.allclose(out[same], ergb[same], atol=dc.MEDIA_TOL, rtol=0)


@pytest.mark.parametrize("depth", [0, 1, 50])
@pytest.mark.parametrize("accel", [0, 1])
def test_every_ray_is_the_probes_path_f32(ctx, scenes, oracle, accel, depth):
    rays, keys, ctr0 = dc.camera_paths(oracle, "cover", N)
    ds = scenes("cover")
    _set(ctx, accel=accel)
    try:
        mean, err, cnt, out = ds.render_rays(rays, 1, keys, ctr0=ctr0, depth=depth, precision="f32", return_rays=True)
        rgb, nseg, _, _ = ds.probe_paths(rays, keys, depth=depth, ctr0=ctr0, precision="f32")
    finally:
        _set(ctx, accel=1)
    assert np.array_equal(out, rgb) and int(cnt[0]) == int(nseg.sum()) and int(cnt[1]) == N
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out) and np.array_equal(mean, out)
    assert (out != ds.probe_paths(rays, keys, depth=depth, ctr0=ctr0)[0]).any() or depth == 0   # (not the f64 kernel's answer)


def test_scan_variants_agree(ctx, scenes, oracle):
    """the LDS-staged scans are answered with the scalar-cache scan: every variant of the flat scan gives the same rays"""
    rays, keys, ctr0 = dc.camera_paths(oracle, "cover", N)
    ds = scenes("cover")
    want = ds.render_rays(rays, 1, keys, ctr0=ctr0, return_rays=True)
    try:
        for v in range(4):
            _set(ctx, accel=0, scan_variant=v)
            assert _equal(ds.render_rays(rays, 1, keys, ctr0=ctr0, return_rays=True), want), v
    finally:
        _set(ctx, accel=1, scan_variant=3)


# ---- 2. derived keys -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, g_first", [(BIG_SEED, 5), (core.RENDER_SEED, 0), (BIG_SEED & 0xFFFFFFFF, 5)])
def test_derived_keys(scenes, oracle, seed, g_first):
    ng, group = 65, 3
    rays = dc.camera_paths(oracle, "cover", N)[0][:ng * group]
    ds = scenes("cover")
    got = ds.render_rays(rays, group, None, seed=seed, ctr0=2, first=g_first, return_rays=True)
    want = ds.render_rays(rays, group, rr.derived_keys(seed, ng, group, g_first), seed=0, ctr0=2, return_rays=True)
    assert _equal(got, want)
    other = ds.render_rays(rays, group, None, seed=BIG_SEED ^ (1 << 40), ctr0=2, first=5, return_rays=True)
    assert seed != BIG_SEED or (other[3] != got[3]).any()     # the high bits of the seed reach the keys


# ---- 3. fold shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("ng, group", [(1, 1), (1, 2), (3, 21), (63, 1), (64, 1), (65, 3), (7, 64), (5, 65)])
def test_fold_shapes(scenes, oracle, ng, group, precision):
    rays, keys, ctr0 = dc.camera_paths(oracle, "cover", N)
    n = ng * group
    mean, err, cnt, out = scenes("cover").render_rays(rays[:n], group, keys[:n], ctr0=ctr0, precision=precision, return_rays=True)
    emean, eerr = rr.fold(out, group, precision)
    assert np.array_equal(mean, emean) and np.array_equal(err, eerr) and int(cnt[1]) == n
    assert group == 1 or (np.isfinite(err).all() and (err > 0).any())


# ---- 4. the frame through the front door ----------------------------------------------------------------------------------------------------------
def _frame_rays(ds, nx, ny, ns, precision):
    """the pinhole rays of every sample of a frame, grouped per pixel in image order, with their keys: pixel() of core.clj:43-51 up to the camera
    ray in the precision of the frame (frame_reference.frame_samples with the device's probe_camera); a pinhole path starts at draw 2"""
    R = fr.REAL[precision]
    ii, jj, ss = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(ns), indexing="ij"))
    keys = fr.sample_keys(dc.SEED, jj * nx + ii, ss)
    u = (ii.astype(np.float32).astype(R) + fr.draws(keys, 0, precision)) / R(nx)
    v = (jj.astype(np.float32).astype(R) + fr.draws(keys, 1, precision)) / R(ny)
    c = ds.probe_camera(np.stack([u, v], 1).astype(np.float64), keys, precision=precision)
    assert (c[:, 7] == 0).all()
    return rr.pixel_major(c[:, :7], nx, ny, ns), rr.pixel_major(keys, nx, ny, ns)


@pytest.mark.parametrize("name, precision", [(n, "f64") for n in rr.SCENES] + [("cover", "f32")])
def test_pinhole_rays_give_the_frame(ctx, scenes, name, precision):
    nx, ny, ns = rr.FRAME
    ds = scenes(rr.pinhole_flat(name))
    rays, keys = _frame_rays(ds, nx, ny, ns, precision)
    mean, err, cnt, _ = ds.render_rays(rays, ns, keys, ctr0=2, depth=dc.FULL, precision=precision)
    lin, _, fcnt = ds.render(nx, ny, ns, dc.FULL, dc.SEED, precision)
    assert np.array_equal(mean.reshape(ny, nx, 3), lin), "%d pixels differ" % (mean.reshape(ny, nx, 3) != lin).any(axis=2).sum()
    assert int(cnt[0]) == int(fcnt[0]) and int(cnt[1]) == nx * ny * ns
    try:
        plin, _, perr, _ = ds.render_progressive(nx, ny, 0, ns, dc.FULL, dc.SEED, precision)
    finally:
        ctx.progressive_release()
    assert np.array_equal(plin, lin) and np.array_equal(err.reshape(ny, nx), perr)


# ---- 5. refill -----------------------------------------------------------------------------------------------------------------------------------
def test_refill_deals_every_lane_more_than_one_ray(oracle):
    """more rays than twice the lanes of the smallest persistent launch the options allow (one workgroup per CU), short and long paths interleaved:
    every lane is dealt rays again and again, next to lanes in the middle of theirs"""
    c = core.Context(0)
    ds = core.DeviceScene(rr.glass_flat(), ctx=c)
    try:
        c.set_option("blocks_per_cu", 1)
        lanes = c.device_info()["compute_units"] * 256
        rays, keys, ctr0 = rr.refill_set(oracle, 2 * lanes + 1)
        assert len(rays) >= 2 * lanes
        mean, err, cnt, out = ds.render_rays(rays, 1, keys, ctr0=ctr0, return_rays=True)
        rgb, nseg, _, _ = ds.probe_paths(rays, keys, ctr0=ctr0)
        assert np.array_equal(out, rgb), "%d of %d rays differ" % ((out != rgb).any(axis=1).sum(), len(rays))
        assert int(cnt[0]) == int(nseg.sum()) and int(cnt[1]) == len(rays)
        base = len(rr.refill_base(oracle)[0])
        assert (nseg[:base] == 1).mean() >= 0.1 and (nseg[:base] >= 4).mean() >= 0.1      # the condition, on the device's own counts
        c.set_option("blocks_per_cu", 8)
        assert _equal(ds.render_rays(rays, 1, keys, ctr0=ctr0, return_rays=True), (mean, err, cnt, out))
    finally:
        ds.close()
        c.close()


# ---- 6. chunks -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_chunks_with_a_state_are_the_one_shot(scenes, oracle, precision):
    ng, group = 37, 12
    rays = dc.camera_paths(oracle, "cover", N)[0][:ng * group].reshape(ng, group, 7)
    ds = scenes("cover")
    whole = rr.new_state(ng)
    mean, err, cnt, out = ds.render_rays(rays.reshape(-1, 7), group, None, seed=BIG_SEED, ctr0=2, precision=precision, state=whole, return_rays=True)
    assert np.array_equal(ds.render_rays(rays.reshape(-1, 7), group, None, seed=BIG_SEED, ctr0=2, precision=precision)[0], mean)   # a state changes no bit
    estate = rr.new_state(ng)
    emean, eerr = rr.fold(out, group, precision, 0, estate)
    assert np.array_equal(mean, emean) and np.array_equal(err, eerr) and np.array_equal(whole, estate)
    for split in ((5, 7), (1, 1, 10)):
        state, first, total = np.full((ng, rr.RAYS_REC), -7.0), 0, np.zeros(2, np.uint64)       # (a record that starts is not read)
        for n in split:
            m, e, c, _ = ds.render_rays(rays[:, first:first + n].reshape(-1, 7), n, None, seed=BIG_SEED, ctr0=2, precision=precision, first=first, state=state)
            first += n
            total += c
        assert np.array_equal(m, mean) and np.array_equal(e, err) and np.array_equal(state, whole) and np.array_equal(total, cnt), split
    # a state continues only with the count it holds: refused, and left as it was
    before = whole.copy()
    with pytest.raises(core.RtmiError) as ei:
        ds.render_rays(rays[:, :5].reshape(-1, 7), 5, None, seed=BIG_SEED, ctr0=2, precision=precision, first=5, state=whole)
    assert ei.value.code == -5 and np.array_equal(whole, before)
    whole[3, 9] = 11.0
    with pytest.raises(core.RtmiError) as ei:
        ds.render_rays(rays[:, :5].reshape(-1, 7), 5, None, seed=BIG_SEED, ctr0=2, precision=precision, first=12, state=whole)
    assert ei.value.code == -5


def test_workspace_passes_change_no_bit(scenes, oracle):
    """the device form without out_rays keeps the radiance in the workspace: option workspace_bytes at its floor splits the call into passes of whole groups"""
    torch = pytest.importorskip("torch")
    ng, group = 9000, 7                                        # 63 000 rays x 24 bytes = 1.5 MB: two passes at 1 MiB
    base = dc.camera_paths(oracle, "cover", N)[0]
    rays = np.tile(base, (21, 1))[:ng * group]
    ds = scenes("cover")
    want = ds.render_rays(rays, group, None, seed=BIG_SEED, ctr0=2, first=3)
    d_rays = torch.from_numpy(rays).cuda()
    outs = []
    try:
        for ws in (1 << 20, 64 << 30):
            ds.ctx.set_option("workspace_bytes", ws)
            mean, err = torch.zeros((ng, 3), dtype=torch.float64, device="cuda"), torch.zeros(ng, dtype=torch.float64, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ds.render_rays_device(ng, group, d_rays, mean, err, seed=BIG_SEED, ctr0=2, first=3, out_counters=cnt)
            assert ds.render_rays(rays[:group], group)[2][1] == group      # a host call on the same context synchronises its stream
            outs.append((mean.cpu().numpy(), err.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64)))
    finally:
        ds.ctx.set_option("workspace_bytes", 64 << 30)
    for got in outs:
        assert _equal(got, want[:3])


# ---- 7. stream and neighbours ----------------------------------------------------------------------------------------------------------------------
def test_device_form_on_a_callers_stream(scenes, oracle):
    torch = pytest.importorskip("torch")
    ng, group = 65, 3
    rays, keys, ctr0 = dc.camera_paths(oracle, "cover", N)
    rays, keys = rays[:ng * group], keys[:ng * group]
    ds = scenes("cover")
    state = rr.new_state(ng)
    host = ds.render_rays(rays, group, keys, ctr0=ctr0, state=state, return_rays=True)
    st = torch.cuda.Stream()
    d_rays, d_keys = torch.from_numpy(rays).cuda(), torch.from_numpy(keys.view(np.int64)).cuda()
    mean, err = torch.full((ng, 3), -1.0, dtype=torch.float64, device="cuda"), torch.full((ng,), -1.0, dtype=torch.float64, device="cuda")
    out, cnt = torch.full((ng * group, 3), -1.0, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    d_state = torch.full((ng, rr.RAYS_REC), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ds.render_rays_device(ng, group, d_rays, mean, err, keys=d_keys, ctr0=ctr0, state=d_state, out_rays=out, out_counters=cnt, stream=st.cuda_stream)
    st.synchronize()
    assert _equal((mean.cpu().numpy(), err.cpu().numpy(), cnt.cpu().numpy().astype(np.uint64), out.cpu().numpy()), host)
    assert np.array_equal(d_state.cpu().numpy(), state)


def test_a_live_progressive_frame_is_not_disturbed(ctx, scenes, oracle):
    nx, ny = 24, 16
    rays, keys, ctr0 = dc.camera_paths(oracle, "cover", N)
    ds = scenes("cover")
    try:
        want = ds.render_progressive(nx, ny, 0, 6)
        ctx.progressive_release()
        ds.render_progressive(nx, ny, 0, 3)
        ds.render_rays(rays, 8, keys, ctr0=ctr0)
        assert ctx.progressive_samples() == 3
        assert _equal(ds.render_progressive(nx, ny, 3, 3), want)
    finally:
        ctx.progressive_release()


def test_edited_scenes_and_the_camera(ctx, oracle):
    """after set_geometry / set_materials / set_camera the call equals one on a scene created fresh from the edited arrays; the camera does not matter"""
    import copy
    rays, keys, ctr0 = dc.camera_paths(oracle, "cover", N)
    f = dc.flat("cover")
    ds = core.DeviceScene(f, ctx=ctx)
    fresh = None
    try:
        before = ds.render_rays(rays, 4, keys, ctr0=ctr0, return_rays=True)
        other = cam.pinhole_camera(lookfrom=np.array([-3.0, 4.0, 9.0]), lookat=np.array([0.0, 0.5, 0.0]), vup=np.array([0.0, 1.0, 0.0]), vfov=55, aspect=1.5)
        ds.set_camera(other)
        assert _equal(ds.render_rays(rays, 4, keys, ctr0=ctr0, return_rays=True), before)
        edit = copy.copy(f)
        edit.prim_mat = np.concatenate([f.prim_mat[:5], np.roll(f.prim_mat[5:], 7)])
        edit.prim_geom = np.array(f.prim_geom, np.float64, copy=True)
        edit.prim_geom[5:, 0] += 0.04 * np.cos(np.arange(len(f.prim_kind) - 5))
        ds.set_materials(edit)
        ds.set_geometry(edit)
        after = ds.render_rays(rays, 4, keys, ctr0=ctr0, return_rays=True)
        assert (after[3] != before[3]).any()
        fresh = core.DeviceScene(ds.flat, ctx=ctx)
        assert _equal(fresh.render_rays(rays, 4, keys, ctr0=ctr0, return_rays=True), after)
        assert np.array_equal(after[3], ds.probe_paths(rays, keys, ctr0=ctr0)[0])
    finally:
        ds.close()
        if fresh is not None:
            fresh.close()


# ---- 8. panorama ---------------------------------------------------------------------------------------------------------------------------------
def test_panorama_inside_the_cornell_box(scenes):
    nx, ny, ns = 32, 16, 4
    eye = np.array([278.0, 278.0, 278.0])
    look = dict(lookfrom=eye, lookat=np.array([278.0, 278.0, 500.0]), vup=np.array([0.0, 1.0, 0.0]))
    ds = scenes("cornell")
    lin, q, err, cnt = ds.render_with(cam.panorama_rays, nx, ny, ns, 3, **look)
    assert _equal(ds.render_with(cam.panorama_rays, nx, ny, ns, 4, **look), (lin, q, err, cnt))
    # ... = the fold of probe_paths over the generator's rays
    rays, ctr0 = cam.panorama_rays(nx, ny, 0, ns, **look)
    keys = rr.derived_keys(core.RENDER_SEED, nx * ny, ns)
    rgb, nseg, log, nlog = ds.probe_paths(rays, keys, ctr0=ctr0, max_seg=1)
    mean, eerr = rr.fold(rgb, ns)
    assert np.array_equal(lin, mean.reshape(ny, nx, 3)[::-1]) and np.array_equal(err, eerr.reshape(ny, nx)[::-1])
    assert np.array_equal(q, fr.quantise(lin)) and int(cnt[0]) == int(nseg.sum()) and int(cnt[1]) == nx * ny * ns
    # Every path hits the box, except through its open front (the plane z = 0, which the reference's box leaves open): a ray from the centre leaves
    # through it if it reaches z = 0 inside 0 < x, y < 555.  All others have a first hit on record; the few that leave end there, black.
    d = rays[:, 3:6]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[:, 2] < 0, -eye[2] / d[:, 2], np.inf)
    px, py = eye[0] + t * d[:, 0], eye[1] + t * d[:, 1]
    may_leave = np.isfinite(t) & (px > 0) & (px < 555) & (py > 0) & (py < 555)
    assert (nlog[~may_leave] == 1).all() and (~may_leave).mean() > 0.8
    gone = nlog == 0
    assert (nseg[gone] == 1).all() and (rgb[gone] == 0).all() and may_leave[gone].all()
    assert (nseg[~gone & (rgb == 0).all(axis=1)] >= 2).all()      # a path that hit and brought nothing back went on past its first segment
    assert (lin > 0).any() and np.isfinite(err).all()


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(ctx, scenes):
    L = _ffi.lib()
    ds, box = scenes("cover"), scenes("cornell")
    rays = np.zeros((6, 7))
    rays[:, 5] = 1.0
    mean, err = np.zeros((6, 3)), np.zeros(6)
    big = np.zeros(1)   # never read: the call is refused before it looks at a row

    def call(handle, precision, ng, group, g_first, depth=50, rays=rays, mean=mean, err=err):
        return L.rtmi_render_rays(handle, precision, ng, group, g_first, _ffi.ptr(rays), None, 7, 0, depth, None, _ffi.ptr(mean), _ffi.ptr(err), None, None)

    idle = C.c_int32()
    core.check(L.rtmi_stream_idle(ctx.handle, C.byref(idle)))
    cases = [((ds.handle, 0, -1, 2, 0), -1), ((ds.handle, 0, 3, 0, 0), -1), ((ds.handle, 0, 3, -2, 0), -1), ((ds.handle, 0, 3, 2, -1), -1),
             ((ds.handle, 0, 3, 2, 0, -1), -1),
             ((ds.handle, 0, 1 << 20, 1 << 11, 0, 50, big), -1),              # 2^31 rays: more than 2^31 - 64
             ((ds.handle, 0, (1 << 31) - 63, 1, 0, 50, big), -1),
             ((ds.handle, 0, 3, 2, (1 << 31) - 2), -1),                        # g_first + group overflows
             ((ds.handle, 0, 3, 2, 0, 50, None), -1), ((ds.handle, 0, 3, 2, 0, 50, rays, None), -1), ((ds.handle, 0, 3, 2, 0, 50, rays, mean, None), -1),
             ((None, 0, 3, 2, 0), -5), ((None, 7, 3, 0, 0), -1),              # arguments before the handle, the handle before the precision
             ((None, 7, 3, 2, 0), -5), ((ds.handle, 7, 3, 2, 0), -1),
             ((box.handle, 1, 3, 2, 0), -3)]                                  # RTMI_F32 on a mixed-kind scene
    for args, code in cases:
        assert call(*args) == code, (args[1:], code, L.rtmi_last_error())
        core.check(L.rtmi_stream_idle(ctx.handle, C.byref(idle)))
        assert idle.value == 1
    assert call(ds.handle, 0, 0, 2, 0) == 0 and call(ds.handle, 0, 0, 2, 0, 50, None, None, None) == 0      # no groups: success, nothing launched
    assert L.rtmi_render_rays_device(None, 0, 3, 2, 0, None, None, 7, 0, 50, None, None, None, None, None, None) == -1
    with pytest.raises(ValueError):
        ds.render_rays(rays[:5], 2)
    with pytest.raises(ValueError):
        ds.render_rays(rays, 2, state=np.zeros((2, rr.RAYS_REC)))
    assert call(ds.handle, 0, 3, 2, 0) == 0 and (mean[:3] == mean[0]).all()
