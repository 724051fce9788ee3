"""Option "defer_emitters": a path that ends on the scene's deferred emitter -- the cover scene's sky dome -- is stored as {attenuation, normal y} and finished
by the fold (reduce_kernel / frame_fold_kernel, DEFER twins) instead of the trace kernel.  The same operations run on the same operands, so every output
must be bit for bit what option 0 gives: every assertion below is np.array_equal on the linear frame, the rgb8 frame and the counters (and the standard-error
plane and the per-tile sample counts where a call has them), between the two settings of the option on ONE scene and context.

The frame is the cover scene at n = 3, 72 x 44 x 8: partial tiles on both edges; tiles that are all sky, mixed, and without sky.  The case at the 1 MiB floor of
"workspace_bytes" renders 32 samples, not 8: a pass holds 1 MiB / (54 tiles x 64 x 3 x 8 B) = 12 samples, so 8 would be ONE pass and the case is there for
several (3 here; the same number under both settings: the budget counts three reals per item whatever the record holds).

Scenes without a deferred emitter (a sky whose gradient reads u, two gradient lights, a constant sky, the Cornell box) run the 3-real path under both settings and
must be equal as well -- and rtmi_last_record_reals says which path a render took: every case asserts 4 reals where the render must defer and 3 where it
must not; so must a live scene after each step of a material edit that takes the deferred emitter away and brings it back, against a fresh scene.
One comparison with the CPU oracle under default options carries the bound of the existing parity tests (RMS < 1e-13, counters equal)."""
import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import core, dist
from raytrace_clj_amd import hitable as hit
from raytrace_clj_amd import shader as shad
from raytrace_clj_amd import texture as tex
from raytrace_clj_amd.util import vec3

pytestmark = pytest.mark.gpu

NX, NY, NS = 72, 44, 8
REGION = (5, 3, 61, 40)  # no edge on a tile border


def _sky(co=(1, 1, 1), cu=(1, 1, 1), cv=(0.5, 0.7, 1.0), cuv=(0.5, 0.7, 1.0)):
    return shad.diffuse_light(tex=tex.uv_gradient(co=vec3(*co), cu=vec3(*cu), cv=vec3(*cv), cuv=vec3(*cuv)))


def _cover(sky=None, extra=(), aperture=None, nx=NX, ny=NY):
    """the cover scene at n = 3 as a Hitlist (item order = primitive order: item 0 is the dome); sky: another material for the dome"""
    sc = r.scene.make_random_scene(nx, ny, 3, False, bvh=False)
    items = list(sc["world"].items)
    assert isinstance(items[0], hit.UVSphere) and items[0].radius == 1000
    if sky is not None:
        items[0] = hit.uv_sphere(center=vec3(0, 0, 0), radius=1000, material=sky)
    camera = sc["camera"]
    if aperture is not None:
        camera = cam.thin_lens_camera(lookfrom=vec3(13, 2, 3), lookat=vec3(0, 0, 0), vup=vec3(0, 1, 0), vfov=20,
                                      aspect=r.scene._aspect(nx, ny), aperture=aperture, focus_dist=10.0, t0=0.0, t1=1.0)
    return {"camera": camera, "world": hit.hitlist(items=items + list(extra))}


SKY_READS_U = dict(co=(1, 1, 1), cu=(0.9, 1, 1), cv=(0.5, 0.7, 1.0), cuv=(0.5, 0.7, 1.0))
SKY_CONSTANT = shad.diffuse_light(tex=tex.constant(color=vec3(0.5, 0.7, 1.0)))


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_ctx():
    c = core.Context(0)
    c.set_option("workspace_bytes", 1 << 20)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cover(ctx):
    ds = core.DeviceScene(_cover(), ctx=ctx)
    yield ds
    ds.close()


def _passes(c):
    import ctypes as C
    v = C.c_int32()
    core.check(r._ffi.lib().rtmi_last_passes(c.handle, C.byref(v)))
    return v.value


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, "output %d differs in %d places" % (k, int((x != y).sum())))


def _reals(c):
    """reals per sample record of the context's last render: 4 = it deferred, 3 = it did not (rtmi_last_record_reals)"""
    import ctypes as C
    v = C.c_int32()
    core.check(r._ffi.lib().rtmi_last_record_reals(c.handle, C.byref(v)))
    return v.value


def _both(c, call, what, defers=True):
    """call() under defer_emitters 1 and 0 on context c -> the outputs (equal).  defers: whether the render under 1 must have taken the deferring
    path (4-real records); under 0 none may."""
    out = []
    for v in (1, 0):
        c.set_option("defer_emitters", v)
        out.append(call())
        assert _reals(c) == (4 if v and defers else 3), (what, "defer_emitters %d: records of %d reals" % (v, _reals(c)))
    c.set_option("defer_emitters", 1)
    _same(out[0], out[1], what)
    return out[0]


def test_cover_frame_and_region(ctx, cover):
    lin, q, cnt = _both(ctx, lambda: cover.render(NX, NY, NS), "frame")
    assert cnt[1] == NX * NY and lin.min() > 0
    rl, rq, rc = _both(ctx, lambda: cover.render(NX, NY, NS, region=REGION), "region")
    x0, y0, x1, y1 = REGION
    assert np.array_equal(rl, lin[y0:y1, x0:x1]) and np.array_equal(rq, q[y0:y1, x0:x1])


def test_cover_many_passes(small_ctx):
    ds = core.DeviceScene(_cover(), ctx=small_ctx)
    try:
        passes = []

        def call():
            out = ds.render(NX, NY, 32)
            passes.append(_passes(small_ctx))
            return out

        _both(small_ctx, call, "1 MiB workspace")
        assert passes[0] == passes[1] == 3, passes
    finally:
        ds.close()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_depth_limits(ctx, cover, depth):
    _both(ctx, lambda: cover.render(NX, NY, NS, depth=depth), "depth %d" % depth)


def test_depth_zero_and_f32(ctx, cover):
    _both(ctx, lambda: cover.render(NX, NY, NS, depth=0), "depth 0")
    _both(ctx, lambda: cover.render(NX, NY, NS, precision="f32"), "f32")
    _both(ctx, lambda: cover.render(NX, NY, NS, precision="f32", region=REGION), "f32 region")


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_larger_tree_sliced_kernels(ctx, cover11, precision, monkeypatch):
    """n = 11 (some 480 spheres: a tree of more than 128 inner nodes and an entry grid): the time-sliced tree kernels, which the frames of n = 3 never
    select (their small tree runs the plain loop) -- first the one with its camera-ray stash in LDS, then (RTMI_SPHERE_LDS_STASH=0, read at every
    render) the one with the stash in registers"""
    ds = core.DeviceScene(cover11, ctx=ctx)
    try:
        assert ds.tree_info()[0] >= 128
        lds = _both(ctx, lambda: ds.render(NX, NY, 4, precision=precision), "n = 11, %s" % precision)
        monkeypatch.setenv("RTMI_SPHERE_LDS_STASH", "0")
        _same(lds, _both(ctx, lambda: ds.render(NX, NY, 4, precision=precision), "n = 11, %s, register stash" % precision), "the two stashes")
    finally:
        ds.close()


def test_flat_scan_and_counting_kernels_do_not_defer(ctx, cover):
    """only the tree kernels have deferring twins: the flat scan and the counting instantiation render the same frame through 3-real records"""
    tree = _both(ctx, lambda: cover.render(NX, NY, NS), "tree")
    ctx.set_option("accel", 0)
    try:
        _same(tree, _both(ctx, lambda: cover.render(NX, NY, NS), "flat scan", defers=False), "flat scan against the tree")
    finally:
        ctx.set_option("accel", 1)
    ctx.set_option("count_traversal", 1)
    try:
        _same(tree, _both(ctx, lambda: cover.render(NX, NY, NS), "counting", defers=False), "counting kernel against the tree")
    finally:
        ctx.set_option("count_traversal", 0)


def test_open_aperture(ctx):
    ds = core.DeviceScene(_cover(aperture=0.5), ctx=ctx)
    try:
        _both(ctx, lambda: ds.render(NX, NY, NS), "aperture 0.5")
    finally:
        ds.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_progressive_three_calls(ctx, cover, precision):
    """1 + 3 + 4 samples; also with the option changed between the calls of one frame (the frame's state has one layout)"""
    def frame(settings):
        outs, k = [], 0
        for v, n in zip(settings, (1, 3, 4)):
            ctx.set_option("defer_emitters", v)
            outs.extend(cover.render_progressive(NX, NY, k, n, precision=precision))
            assert _reals(ctx) == (4 if v else 3)
            k += n
        ctx.set_option("defer_emitters", 1)
        ctx.progressive_release()
        return outs

    on = frame((1, 1, 1))
    _same(on, frame((0, 0, 0)), "progressive")
    _same(on, frame((1, 0, 1)), "progressive, option toggled")
    one = _both(ctx, lambda: cover.render(NX, NY, 8, precision=precision), "one shot")
    _same(on[8:10] + on[11:12], one, "progressive against one shot")


def test_adaptive_two_rounds(ctx, cover):
    def rounds():
        outs = []
        for k, n in ((0, 4), (4, 4)):
            outs.extend(cover.render_adaptive(NX, NY, k, n, 0.02))
            outs.append(np.asarray(ctx.adaptive_status()))
            outs.append(ctx.adaptive_active_tiles())
        ctx.progressive_release()
        return outs

    out = _both(ctx, rounds, "adaptive")
    smp = out[3 + 7]  # the second round's per-pixel sample counts
    assert smp.min() == 4 and smp.max() == 8, "eps must retire some tiles after the first round and keep others"


def test_two_replicas_one_device():
    md = dist.MultiDevice(r.flatten.flatten(_cover()), [0, 0])
    try:
        out = []
        for v in (1, 0):
            md.set_option("defer_emitters", v)
            out.append(md.render(NX, NY, NS))
            assert [_reals(c) for c in md.ctxs] == [4 if v else 3] * 2
        _same(out[0], out[1], "two replicas")
    finally:
        md.close()


def _two_spheres(reads_u):
    sc = r.scene.make_two_spheres(NX, NY)
    if not reads_u:
        return sc
    items = [hit.uv_sphere(center=vec3(0, 0, 0), radius=1000, material=_sky(**SKY_READS_U)),
             hit.sphere(center=vec3(0, -10, 0), radius=10, material=shad.lambertian(albedo=tex.constant(color=vec3(0.4, 0.5, 0.3)))),
             hit.uv_sphere(center=vec3(0, 2, 0), radius=2, material=shad.lambertian(albedo=tex.uv_gradient(co=vec3(0, 1, 0), cu=vec3(0, 1, 1), cv=vec3(1, 0, 1), cuv=vec3(1, 0, 0))))]
    return {"camera": sc["camera"], "world": hit.hitlist(items=items)}


@pytest.mark.parametrize("name", ["two-spheres", "two-spheres-sky-reads-u", "cover-sky-reads-u", "cover-two-gradient-lights", "cover-constant-sky", "cornell"])
def test_other_scenes(ctx, name):
    """two-spheres has a deferred emitter (its sky does not vary with u); the others have none and keep the 3-real path under both settings"""
    nx, ny, ns = NX, NY, NS
    if name.startswith("two-spheres"):
        sc = _two_spheres(name.endswith("reads-u"))
    elif name == "cover-sky-reads-u":
        sc = _cover(sky=_sky(**SKY_READS_U))
    elif name == "cover-two-gradient-lights":
        sc = _cover(extra=[hit.uv_sphere(center=vec3(-2, 1.5, 2), radius=0.6, material=_sky(cv=(4, 2, 1), cuv=(4, 2, 1)))])
    elif name == "cover-constant-sky":
        sc = _cover(sky=SKY_CONSTANT)
    else:
        nx, ny, ns = 48, 48, 4
        sc = r.scene.make_cornell_box(nx, ny)
    ds = core.DeviceScene(sc, ctx=ctx)
    try:
        lin, q, cnt = _both(ctx, lambda: ds.render(nx, ny, ns), name, defers=name == "two-spheres")
        assert cnt[1] == nx * ny
    finally:
        ds.close()


@pytest.mark.parametrize("stream", [None, 0])
def test_live_material_edit(ctx, stream):
    """constant sky -> a gradient that reads u -> the first sky again: after each step the live scene renders what a fresh scene renders, under both settings"""
    steps = [_cover(sky=SKY_CONSTANT), _cover(sky=_sky(**SKY_READS_U)), _cover()]
    live = core.DeviceScene(_cover(), ctx=ctx)
    try:
        for k, sc in enumerate(steps):
            rebuilt = live.set_materials(sc, stream=stream)
            assert not rebuilt
            got = _both(ctx, lambda: live.render(NX, NY, NS), "live, step %d" % k, defers=k == 2)
            fresh = core.DeviceScene(sc, ctx=ctx)
            try:
                _same(got, _both(ctx, lambda: fresh.render(NX, NY, NS), "fresh, step %d" % k, defers=k == 2), "live against fresh, step %d" % k)
            finally:
                fresh.close()
    finally:
        live.close()


def test_against_the_oracle(ctx, oracle):
    nx, ny, ns = 64, 64, 4
    sc = _cover(nx=nx, ny=ny)
    ds = core.DeviceScene(sc, ctx=ctx)
    try:
        lin, q, cnt = ds.render(nx, ny, ns)  # default options
        assert _reals(ctx) == 4
    finally:
        ds.close()
    exp, exp8, ecnt = oracle.render(r.flatten.flatten(sc), nx, ny, ns, core.DEFAULT_DEPTH, core.RENDER_SEED, nthreads=16)
    rms = float(np.sqrt(np.mean((lin - exp) ** 2)))
    print("RMS against the oracle: %.3g" % rms)
    assert rms < 1e-13
    assert np.array_equal(np.asarray(cnt, np.uint64), np.asarray(ecnt, np.uint64))
