"""The timing intervals of the caller-supplied ray calls on a Context(timing=True): every persistent-queue launch is one interval of
last_trace_ms(), and its reduce part (last_reduce_ms()) ends behind the fold that follows the kernel, or at once where no fold follows.  So a call
reports one interval per launch of its passes: the counts below are read off the launch sequence of each call, not measured."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import hitable as hit
from raytrace_clj_amd import shader as shad
from raytrace_clj_amd import texture as tex
from raytrace_clj_amd.util import SplitMix64, vec3

NX, NY = 16, 8  # 128 pixel-centre rays: two waves
PASS_GROUP = 30000  # rays (or light samples) per group: 24 B each, so option "workspace_bytes" at its 1 MiB floor holds one group per pass


def _scene():
    """a ground, a ball and a constant-emission lamp above them"""
    grey = shad.lambertian(albedo=tex.constant(color=vec3(0.5, 0.5, 0.5)))
    lamp = shad.diffuse_light(tex=tex.constant(color=vec3(5.0, 4.0, 3.0)))
    items = [hit.sphere(center=vec3(0, -1000, 0), radius=1000, material=grey),
             hit.sphere(center=vec3(0, 1, 0), radius=1, material=grey),
             hit.sphere(center=vec3(0.5, 5, 1), radius=1.5, material=lamp)]
    return {"camera": r.camera.thin_lens_camera(lookfrom=vec3(6, 3, 9), lookat=vec3(0, 1, 0), vup=vec3(0, 1, 0), vfov=35, aspect=float(NX) / float(NY),
                                                aperture=0.0, focus_dist=10.0, t0=0.0, t1=1.0),
            "world": hit.make_bvh(items, 0.0, 1.0, SplitMix64(0x11A7))}


@functools.lru_cache(maxsize=None)
def _open():
    """one timed context and scene for the module, and the view's rays and first hits"""
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene(), ctx=ctx)
    assert len(ds.lights()) == 1
    rays = ds.pixel_centre_rays(NX, NY)
    hits = ds.query_hits(rays)
    assert 0 < np.count_nonzero(hits[:, 0]) < len(hits)
    return ctx, ds, rays, hits


def _intervals(ctx, call):
    """the window of one call: (trace intervals, reduce intervals), after checking that both sums are finite and not negative"""
    ctx.last_trace_ms()  # (closes whatever window earlier calls left open)
    call()
    trace_ms, n_trace = ctx.last_trace_ms()
    reduce_ms, n_reduce = ctx.last_reduce_ms()
    assert math.isfinite(trace_ms) and trace_ms >= 0.0 and math.isfinite(reduce_ms) and reduce_ms >= 0.0, (trace_ms, reduce_ms)
    return n_trace, n_reduce


def _ao_device(ds):
    import torch
    dev = torch.device("cuda", 0)
    vis = torch.zeros(NX * NY, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ds.ambient_occlusion_device(NX, NY, 4, 2.0, out_visibility=vis)
    torch.cuda.synchronize(dev)


CALLS = {
    "render_rays": (1, lambda ds, rays, hits: ds.render_rays(rays, group=4, depth=8)),
    "query_hits": (1, lambda ds, rays, hits: ds.query_hits(rays)),
    "occluded": (1, lambda ds, rays, hits: ds.occluded(rays, group=4)),
    "occlusion_hemisphere": (1, lambda ds, rays, hits: ds.occlusion_hemisphere(hits, 4, view=rays)),
    "occlusion_targets": (1, lambda ds, rays, hits: ds.occlusion_targets(hits, [[0.5, 5.0, 1.0], [6.0, 3.0, 9.0]], view=rays)),
    "ambient_occlusion_device": (2, lambda ds, rays, hits: _ao_device(ds)),  # the first hits, then the hemisphere rays
    "direct_irradiance": (1, lambda ds, rays, hits: ds.direct_irradiance(hits, 4, view=rays)),
    "render_direct": (2, lambda ds, rays, hits: ds.render_direct(NX, NY, 4)),  # the first hits, then one light pass
    "render_rays_nee": (1, lambda ds, rays, hits: ds.render_rays_nee(rays, group=4, depth=8)),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_one_interval_per_launch(name):
    ctx, ds, rays, hits = _open()
    expected, call = CALLS[name]
    assert _intervals(ctx, lambda: call(ds, rays, hits)) == (expected, expected)


PASS_CALLS = {
    "render_rays": lambda ds, rays, hits: ds.render_rays(np.tile(rays[:1], (3 * PASS_GROUP, 1)), group=PASS_GROUP, depth=4),
    "render_rays_nee": lambda ds, rays, hits: ds.render_rays_nee(np.tile(rays[:1], (3 * PASS_GROUP, 1)), group=PASS_GROUP, depth=4),
    "direct_irradiance": lambda ds, rays, hits: ds.direct_irradiance(hits[hits[:, 0] != 0.0][:3], PASS_GROUP),
}


@pytest.mark.parametrize("name", sorted(PASS_CALLS))
def test_one_interval_per_workspace_pass(name):
    """three groups (points) whose radiance (contributions) the workspace holds one at a time: three passes, each a launch and its fold.  That the
    passes change no bit of the results is pinned where each call's other properties are (test_gpu_rays, test_gpu_nee, test_gpu_direct)."""
    ctx, ds, rays, hits = _open()
    assert 2 * PASS_GROUP * 24 > (1 << 20) >= PASS_GROUP * 24
    try:
        ctx.set_option("workspace_bytes", 1 << 20)
        assert _intervals(ctx, lambda: PASS_CALLS[name](ds, rays, hits)) == (3, 3)
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
