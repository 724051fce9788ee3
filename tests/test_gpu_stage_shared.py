"""Every host form stages through ONE buffer of the context (HostIo over c->io in rtmi.hip).  What that sharing newly allows to go wrong is checked
here on the small cover scene at 21 x 13 pixels and 4 samples: one context starts a progressive frame with samples [0, 2), then runs a region
render, the feature pass, the denoiser, a reprojection, caller-supplied rays in two chunks, two probes and a retirement by a host noise map -- in an
order in which the arena is small, then at its largest, then small again -- and finishes the frame with samples [2, 4).

  * every result equals, bit for bit, the same call alone on a fresh context;
  * the finished frame equals the frame of a context that ran nothing in between (start, the retirement, the continuation): the frame's state
    does not live in the arena;
  * a second pass repeats the denoiser without its standard error and the rays without keys, records and per-ray radiance, after calls that gave
    them: a plane left out must be absent, not a stale pointer to what the call before left there.

The retirement stands between the two halves of the frame and retires the tiles right of x = 8 (its map is below eps there), so the number it
returns and the sample counts of the finished frame depend on the map having reached the device; the frame therefore continues with render_adaptive
(eps = 0), which is what continues a frame with retired tiles."""
import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import vec3

pytestmark = pytest.mark.gpu

NX, NY, NS, DEPTH, SEED = 21, 13, 4, 8, 0x5EED0002
REGION = (3, 2, 17, 11)
VX, VY = 7, 5  # the two tiny views of the reprojection


def _inputs(scene):
    """the host arrays of the image operations and the rays: fixed pseudo-random values, made once"""
    g = np.random.default_rng(20240607)
    a = {}
    a["dn"] = (g.uniform(0, 1, (NY, NX, 3)), g.uniform(0.01, 0.2, (NY, NX)), g.uniform(0, 1, (NY, NX, 8)))
    cam0 = fl.flatten_camera(scene["camera"])
    cam1 = fl.flatten_camera(cam.thin_lens_camera(lookfrom=vec3(12.6, 2.3, 3.5), lookat=vec3(0, 0, 0), vup=vec3(0, 1, 0), vfov=20, aspect=VX / VY,
                                                  aperture=0.0, focus_dist=10.0, t0=0.0, t1=1.0))
    view = lambda: (g.uniform(0, 1, (VY, VX, 3)), g.uniform(0.01, 0.2, (VY, VX)), g.uniform(0, 1, (VY, VX, 8)))
    a["rp"] = (cam0, cam1, view(), g.uniform(1, 6, (VY, VX)), view())
    n = 5 * 3  # 5 groups of 3 rays towards the scene, given as chunks of 2 and 1 per group
    d = -np.array([13.0, 2.0, 3.0]) + g.uniform(-1.5, 1.5, (n, 3))
    rays = np.concatenate([np.tile([13.0, 2.0, 3.0], (n, 1)), d / np.linalg.norm(d, axis=1, keepdims=True), g.uniform(0, 1, (n, 1))], axis=1)
    a["rays"] = rays.reshape(5, 3, 7)
    a["keys"] = g.integers(0, 2 ** 63, (5, 3), dtype=np.uint64)
    a["probe"] = rays[:7]
    noise = np.full((NY, NX), 1.0)
    noise[:, 8:] = 0.001
    a["noise"] = noise
    return a


def _calls(a, precision):
    """name -> f(ctx, ds): each host form once, with every optional array given"""
    lin, se, ft = a["dn"]
    cam0, cam1, (pl, ps, pf), pw, (cl, cs, cf) = a["rp"]

    def rays_two_chunks(ctx, ds):
        state = np.zeros((5, r._ffi.RAYS_REC))
        first = ds.render_rays(a["rays"][:, :2].reshape(-1, 7), group=2, keys=a["keys"][:, :2].reshape(-1), depth=DEPTH, precision=precision, first=0,
                               state=state, return_rays=True)
        mid = state.copy()
        second = ds.render_rays(a["rays"][:, 2:].reshape(-1, 7), group=1, keys=a["keys"][:, 2:].reshape(-1), depth=DEPTH, precision=precision, first=2,
                                state=state, return_rays=True)
        return first + (mid,) + second + (state,)

    return {
        "render-region": lambda ctx, ds: ds.render(NX, NY, NS, DEPTH, SEED, precision, region=REGION),
        "features": lambda ctx, ds: ds.render_features(NX, NY, 3, SEED, precision, region=REGION),
        "denoise": lambda ctx, ds: ctx.denoise(lin, se, ft, iterations=2),
        "reproject": lambda ctx, ds: ctx.reproject(cam0, cam1, pl, pw, ps, pf, cl, cs, cf, 4.0, sigma_d=0.1, sigma_n=0.3, sigma_a=0.2),
        "rays": rays_two_chunks,
        "probe-hit": lambda ctx, ds: (ds.probe_hit(a["probe"], precision=precision),),
        "probe-paths": lambda ctx, ds: ds.probe_paths(a["probe"], a["keys"].reshape(-1)[:7], depth=DEPTH, max_seg=3, precision=precision),
        # the second pass: the same entries with optional arrays left out
        "denoise-plain": lambda ctx, ds: ctx.denoise(lin, None, None, iterations=1),
        "rays-plain": lambda ctx, ds: ds.render_rays(a["rays"].reshape(-1, 7), group=3, seed=SEED, depth=DEPTH, precision=precision),
    }


# small first, then the largest (the denoiser's sixteen planes of the frame's size), then small again; the rays' two chunks are one entry
ORDER = ("probe-hit", "render-region", "denoise", "probe-paths", "features", "reproject", "rays")
SECOND_PASS = ("denoise-plain", "rays-plain", "denoise", "probe-hit")


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        if g is None or e is None:
            assert g is None and e is None, (what, k)
        else:
            assert g.dtype == e.dtype and np.array_equal(g, e, equal_nan=g.dtype.kind == "f"), (what, "result %d differs" % k)


def _fresh(scene, f):
    """f(ctx, ds) on a context of its own"""
    ctx = core.Context(0)
    try:
        ds = core.DeviceScene(scene, ctx=ctx)
        try:
            return f(ctx, ds)
        finally:
            ds.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_host_forms_share_one_arena(cover_small, precision):
    a = _inputs(cover_small)
    calls = _calls(a, precision)
    alone = {name: _fresh(cover_small, f) for name, f in calls.items()}

    def frame(ctx, ds, between):
        start = ds.render_progressive(NX, NY, 0, 2, DEPTH, SEED, precision)
        got = between(ctx, ds, ORDER)
        retired = ctx.adaptive_retire(a["noise"], 0.5)
        end = ds.render_adaptive(NX, NY, 2, 2, 0.0, DEPTH, SEED, precision)
        return start, retired, end, got, between(ctx, ds, SECOND_PASS)

    plain_start, plain_retired, plain_end, _, _ = _fresh(cover_small, lambda ctx, ds: frame(ctx, ds, lambda *_: {}))
    assert plain_retired == 4  # the 3 x 2 tiles of the frame but the left column
    assert set(np.unique(plain_end[3][:, :8])) == {4} and set(np.unique(plain_end[3][:, 8:])) == {2}

    run = lambda ctx, ds, names: {name: calls[name](ctx, ds) for name in names}
    start, retired, end, got, again = _fresh(cover_small, lambda ctx, ds: frame(ctx, ds, run))
    for name in ORDER:
        _same(got[name], alone[name], name)
    for name in SECOND_PASS:
        _same(again[name], alone[name], "second pass: " + name)
    _same(start, plain_start, "the frame's first half")
    assert retired == plain_retired
    _same(end, plain_end, "the finished frame against the uninterrupted one")
