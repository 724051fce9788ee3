"""Path tracing with next-event estimation on the device (rtmi_render_rays_nee*, rtmi_probe_paths_nee).  The probe's log must equal rtmi_probe_paths'
on the path itself, camera.nee_samples on the light samples, rtmi_query_occluded_device and the oracle on the shadow flags, and the NEE rule's fold
(tests/nee_reference.py) on contributions, radiance and the dropped closing emission -- all as exact doubles; the render must equal the probe; chunks,
passes and the neighbouring cases must change no bit; and the estimate must have the plain path tracer's expectation."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from raytrace_clj_amd import _ffi, camera, core
from tests import direct_cases as dcs
from tests import direct_reference as dref
from tests import nee_cases as ncs
from tests import nee_reference as nref

N = dcs.N_POINTS  # 1 500 view rays: 23 1/2 waves
bits = nref.bits


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


@functools.lru_cache(maxsize=None)
def _open(name):
    """one context and device scene per recipe for the whole module"""
    ctx = core.Context(0)
    return ctx, core.DeviceScene(dcs.flat(name), ctx=ctx)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _inputs(name):
    return dcs.view_rays(_oracle(), name), ncs.path_keys()


def _occluded(ds, rays, precision):
    """occluded_device on host rays, uploaded, range "up to the light" """
    import torch
    if len(rays) == 0:
        return np.zeros(0, np.uint8)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to(_dev())
    d_flags = torch.zeros(len(rays), dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.occluded_device(len(rays), 1, d_rays, out_occluded=d_flags, t_min=nref.T_MIN, t_max=nref.T_MAX, precision=precision)
    torch.cuda.synchronize(_dev())
    return d_flags.cpu().numpy()


def _device_render(ds, call, n_groups, group, rays, keys=None, n_counters=4, state=None, want_rays=True, **kw):
    """one render_rays_device / render_rays_nee_device call on HBM buffers -> (mean, stderr, counters, radiance or None, state or None) on the host"""
    import torch
    n = n_groups * group
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to(_dev())
    d_keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(_dev()) if keys is not None else None
    d_mean = torch.full((n_groups, 3), -7.0, dtype=torch.float64, device=_dev())
    d_se = torch.full((n_groups,), -7.0, dtype=torch.float64, device=_dev())
    d_out = torch.full((n, 3), -7.0, dtype=torch.float64, device=_dev()) if want_rays else None
    d_cnt = torch.full((n_counters,), 9, dtype=torch.int64, device=_dev())
    d_state = torch.from_numpy(state).to(_dev()) if state is not None else None
    torch.cuda.synchronize(_dev())
    getattr(ds, call)(n_groups, group, d_rays, d_mean, d_se, keys=d_keys, state=d_state, out_rays=d_out, out_counters=d_cnt, **kw)
    torch.cuda.synchronize(_dev())
    return (d_mean.cpu().numpy(), d_se.cpu().numpy(), d_cnt.cpu().numpy().tolist(), d_out.cpu().numpy() if want_rays else None,
            d_state.cpu().numpy() if state is not None else None)


def _check_log(name, precision, ds, rays, keys, depth, lights):
    """rtmi_probe_paths_nee against the device's own parts and the rule's fold -> (radiance, states of the light-sampled vertices, segment counts)"""
    f = dcs.flat(name)
    table = camera.light_table(f, lights)
    max_seg = depth + 1
    what = "%s %s depth %d" % (name, precision, depth)
    rgb0, nseg0, log0, nlog0 = ds.probe_paths(rays, keys, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)
    rgb, nseg, log, nlog, drop = ds.probe_paths_nee(rays, keys, lights=lights, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)
    # the path itself is the plain path
    assert np.array_equal(bits(log[:, :, :12]), bits(log0)), what
    assert np.array_equal(nseg, nseg0) and np.array_equal(nlog, nlog0), what
    # step 1: where; steps 2 - 4: which light, the ray, the weight
    at = nref.vertices(f, log, nlog)
    assert np.array_equal(log[:, :, 12] != 0.0, at), what
    i, j, l, d, w, built = nref.samples(log, at, keys, table)
    assert np.array_equal(log[i, j, 13], l.astype(np.float64)), what
    assert np.array_equal(bits(log[i, j, 14:17]), bits(d)) and np.array_equal(bits(log[i, j, 17]), bits(w)), what
    state = log[i, j, 12]
    assert np.array_equal(state == 3.0, ~built), what
    # step 5: the shadow flags are the any-hit query's on those rays, and the oracle's
    shadow = nref.shadow_rays(log, i, j, d, rays[:, 6])[built]
    flags = _occluded(ds, shadow, precision)
    assert np.array_equal(state[built] == 2.0, flags == 1), what
    if precision == "f64" and len(shadow):
        assert np.array_equal(_oracle().probe_hit(f, shadow, tmin=nref.T_MIN, tmax=nref.T_MAX)[:, 0] != 0.0, flags == 1), what
    # T, the contributions and their fold, the closing emission, the radiance
    T = nref.attenuations(f, log, nlog, np.float32 if precision == "f32" else np.float64)
    assert np.array_equal(bits(log[i, j, 18:21]), bits(T[i, j])), what
    contrib, accum = nref.fold(len(rays), max_seg, i, j, l, w, state == 1.0, T, table)
    assert np.array_equal(bits(log[:, :, 21:24]), bits(contrib)), what
    want_drop = nref.dropped(log, nlog, nseg, at, lights)
    assert np.array_equal(drop != 0, want_drop), what
    assert np.array_equal(bits(rgb), bits(accum + np.where(want_drop[:, None], 0.0, rgb0))), what
    return rgb, state, nseg, want_drop


# ---- 1. the probe against the device's own parts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_probe_against_the_devices_own_parts(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    lights = dref.eligible(dcs.flat(name))
    assert ds.lights().tolist() == lights.tolist() and len(lights) >= 1
    seen = set()
    for depth in ncs.DEPTHS:
        rgb, state, nseg, drop = _check_log(name, precision, ds, rays, keys, depth, lights)
        if depth == 0:
            assert len(state) == 0 and (nseg <= 1).all()  # no scatter, no light sample: the closing emission alone
        else:
            seen |= set(state.tolist())
            assert drop.any() and not drop.all()
    assert {1.0, 2.0, 3.0} <= seen  # unoccluded, occluded and unbuilt samples all occur


# ---- 2. the render against the probe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_render_equals_probe(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    lights = dref.eligible(dcs.flat(name))
    for depth in (3, 50):
        rgb, nseg, log, nlog, _ = ds.probe_paths_nee(rays, keys, depth=depth, ctr0=2, max_seg=depth + 1, precision=precision)
        state = log[:, :, 12]
        want = [int(nseg.sum()), N, int(((state == 1.0) | (state == 2.0)).sum()), int((state == 2.0).sum())]
        mean, se, cnt, out, _ = _device_render(ds, "render_rays_nee_device", N // 4, 4, rays, keys, ctr0=2, depth=depth, precision=precision)
        assert np.array_equal(bits(out), bits(rgb)) and cnt == want and want[2] > want[3] > 0, (name, precision, depth, cnt, want)
        h_mean, h_se, h_cnt, h_out = ds.render_rays_nee(rays, 4, lights=lights, keys=keys, ctr0=2, depth=depth, precision=precision, return_rays=True)
        assert np.array_equal(bits(h_out), bits(rgb)) and h_cnt.tolist() == want
        assert np.array_equal(bits(h_mean), bits(mean)) and np.array_equal(bits(h_se), bits(se))


# ---- 3. chunks and passes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_chunks_give_the_bits_of_one_call(name, precision):
    ctx, ds = _open(name)
    ng, group = 60, 25
    rays = _inputs(name)[0].reshape(ng, group, 7)
    whole = np.zeros((ng, _ffi.RAYS_REC))
    one = _device_render(ds, "render_rays_nee_device", ng, group, rays.reshape(-1, 7), seed=99, depth=8, precision=precision, first=0, state=whole)
    state, total, first = np.zeros((ng, _ffi.RAYS_REC)), np.zeros(4, np.int64), 0
    for size in (1, 7, group - 8):
        part = _device_render(ds, "render_rays_nee_device", ng, size, np.ascontiguousarray(rays[:, first:first + size]).reshape(-1, 7), seed=99, depth=8,
                              precision=precision, first=first, state=state)
        state, first, total = part[4], first + size, total + np.array(part[2])
    assert first == group
    assert np.array_equal(bits(part[0]), bits(one[0])) and np.array_equal(bits(part[1]), bits(one[1])) and np.array_equal(bits(state), bits(one[4]))
    assert total.tolist() == [one[2][0], ng * group, one[2][2], one[2][3]] and one[2][1] == ng * group and one[2][2] > 0


@pytest.mark.parametrize("name", ("cornell", "sphere-lamp"))
def test_workspace_passes_change_no_bit(name):
    """without out_rays the radiance lives in the workspace: option workspace_bytes at its floor splits the call into passes of whole groups"""
    ctx, ds = _open(name)
    ng, group = 9000, 7  # 63 000 rays x 24 bytes = 1.5 MB: two passes at 1 MiB
    rays = np.tile(_inputs(name)[0], (42, 1))
    outs = []
    try:
        for ws in (1 << 20, 64 << 30):
            ctx.set_option("workspace_bytes", ws)
            outs.append(_device_render(ds, "render_rays_nee_device", ng, group, rays, seed=5, ctr0=2, depth=6, first=3, want_rays=False)[:3])
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1])) and outs[0][2] == outs[1][2]
    assert outs[0][2][1] == ng * group and outs[0][2][2] > 0


# ---- 4. the neighbouring cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_no_lights_is_render_rays(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    plain = _device_render(ds, "render_rays_device", N // 4, 4, rays, keys, n_counters=2, ctr0=2, depth=50, precision=precision)
    none = _device_render(ds, "render_rays_nee_device", N // 4, 4, rays, keys, lights=[], ctr0=2, depth=50, precision=precision)
    assert all(np.array_equal(bits(none[k]), bits(plain[k])) for k in (0, 1, 3)) and none[2] == plain[2] + [0, 0]
    some = _device_render(ds, "render_rays_nee_device", N // 4, 4, rays, keys, ctr0=2, depth=50, precision=precision)
    assert not np.array_equal(bits(some[3]), bits(plain[3])) and some[2][:2] == plain[2]  # (the paths themselves are the same paths)


def test_a_scene_without_eligible_lights_is_render_rays():
    ctx = core.Context(0)
    ds = core.DeviceScene(dcs.not_lights()["moving"], ctx=ctx)  # its lamp moves: it shines, but it is no light for these calls
    rays, keys = _inputs("sphere-lamp")
    assert len(ds.lights()) == 0
    plain = _device_render(ds, "render_rays_device", N, 1, rays, keys, n_counters=2, ctr0=2, depth=50)
    none = _device_render(ds, "render_rays_nee_device", N, 1, rays, keys, ctr0=2, depth=50)
    assert all(np.array_equal(bits(none[k]), bits(plain[k])) for k in (0, 1, 3)) and none[2] == plain[2] + [0, 0] and plain[3].any()
    ds.close(); ctx.close()


def test_a_listed_subset_keeps_the_unlisted_lamps_emission():
    name = "example-light"
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    both = dref.eligible(dcs.flat(name))
    assert len(both) == 2
    for listed in (both[:1], both[1:]):
        rgb, state, nseg, drop = _check_log(name, "f64", ds, rays, keys, 50, listed)  # (the rule's dropped() compares with the listed lamp alone)
        all_drop = ds.probe_paths_nee(rays, keys, lights=both, depth=50, ctr0=2)[4] != 0
        assert drop.any() and (all_drop & ~drop).any() and not (drop & ~all_drop).any()  # paths that end on the other lamp keep what it emits
        out = _device_render(ds, "render_rays_nee_device", N, 1, rays, keys, lights=listed, ctr0=2, depth=50)[3]
        assert np.array_equal(bits(out), bits(rgb))


def test_a_material_edit_that_switches_the_lamp_off_is_followed():
    from raytrace_clj_amd import flatten as fl
    from raytrace_clj_amd import hitable as hit
    from raytrace_clj_amd.util import vec3
    ctx = core.Context(0)
    ds = core.DeviceScene(dcs.flat("sphere-lamp"), ctx=ctx)
    rays, keys = _inputs("sphere-lamp")
    lit = _device_render(ds, "render_rays_nee_device", N, 1, rays, keys, ctr0=2, depth=50)
    assert len(ds.lights()) == 1 and lit[2][2] > 0
    dark = fl.flatten(dcs.sphere_lamp_scene(lamp=lambda m: hit.sphere(center=vec3(0.5, 5, 1), radius=1.5, material=dcs.shad.lambertian(
        albedo=dcs.tex.constant(color=vec3(0.3, 0.3, 0.3))))))
    ds.set_materials(dark)
    assert len(ds.lights()) == 0
    off = _device_render(ds, "render_rays_nee_device", N, 1, rays, keys, ctr0=2, depth=50)
    plain = _device_render(ds, "render_rays_device", N, 1, rays, keys, n_counters=2, ctr0=2, depth=50)
    assert np.array_equal(bits(off[3]), bits(plain[3])) and off[2] == plain[2] + [0, 0] and not off[3].any()
    ds.close(); ctx.close()


# ---- 5. errors and zero work ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_zero_work():
    L = _ffi.lib()
    ctx = core.Context(0)
    smoke = core.DeviceScene(ncs.media_flat(), ctx=ctx)
    _, ds = _open("sphere-lamp")
    rays = np.ascontiguousarray(_inputs("sphere-lamp")[0][:8])
    mean, se, cnt = np.full((8, 3), -7.0), np.full(8, -7.0), np.full(4, 9, np.uint64)
    lamp = np.asarray(ds.lights(), np.int32)

    def call(scene, n_groups=8, group=1, g_first=0, depth=5, n_lights=0, prims=None, precision=0, r=rays, m=mean):
        return L.rtmi_render_rays_nee(scene.handle, precision, n_groups, group, g_first, core.ptr(r), None, 1, 0, depth, n_lights, core.ptr(prims), None,
                                      core.ptr(m), core.ptr(se), None, core.ptr(cnt))
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)
    # rtmi_render_rays' own errors come first, in their order, whatever the lights and the scene are
    assert call(smoke, n_groups=-1, n_lights=len(many), prims=many) == -1
    assert call(smoke, group=0) == -1 and call(smoke, g_first=-1) == -1 and call(smoke, depth=-1) == -1
    assert call(smoke, r=None, n_lights=len(many), prims=many) == -1 and call(smoke, m=None) == -1
    assert call(smoke, precision=7, n_lights=len(many), prims=many) == -1
    assert call(smoke, precision=1) == -3                                       # (RTMI_F32 on a mixed-kind scene, as rtmi_render_rays)
    # then the list's length, then the media, then the list's entries
    assert call(smoke, n_lights=len(many), prims=many) == -1 and call(smoke, n_lights=-1, prims=many) == -1
    assert call(smoke) == -3 and call(smoke, n_lights=1, prims=np.array([0], np.int32)) == -3
    assert b"ConstantMedium" in L.rtmi_last_error()
    assert call(ds, n_lights=1, prims=np.array([0], np.int32)) == -1 and call(ds, n_lights=1, prims=np.array([10 ** 6], np.int32)) == -1
    assert (mean == -7.0).all() and (se == -7.0).all() and (cnt == 9).all()         # a failed call writes nothing
    # zero work succeeds, on any scene, and writes nothing
    assert call(smoke, n_groups=0) == 0 and call(ds, n_groups=0, r=None, m=None) == 0 and (cnt == 9).all()
    assert call(ds, n_lights=1, prims=lamp) == 0 and cnt[1] == 8 and (mean != -7.0).all()
    # the probe refuses the same scene, and the python layer raises
    with pytest.raises(core.RtmiError) as ei:
        smoke.probe_paths_nee(rays, np.arange(8, dtype=np.uint64))
    assert ei.value.code == -3
    with pytest.raises(core.RtmiError) as ei:
        smoke.render_rays_nee(rays)
    assert ei.value.code == -3
    smoke.close(); ctx.close()


# ---- 6. the same estimand, on the device ---------------------------------------------------------------------------------------------------------
def test_same_estimand_on_the_device():
    """test_nee_host.test_same_estimand's inputs, counts (G = 48, n = 4096) and conditions, with render_rays_device as the plain side"""
    ctx, ds = _open(ncs.ESTIMAND_SCENE)
    rays, keys = ncs.estimand_inputs(_oracle())
    G, n = ncs.ESTIMAND_G, ncs.ESTIMAND_N
    plain = _device_render(ds, "render_rays_device", G, n, rays, keys, n_counters=2, depth=ncs.ESTIMAND_DEPTH)[3]
    nee = _device_render(ds, "render_rays_nee_device", G, n, rays, keys, depth=ncs.ESTIMAND_DEPTH)[3]
    z = nref.z_scores(plain.reshape(G, n, 3), nee.reshape(G, n, 3))
    print("z: mean %.3f (bound %.3f), max |z| %.3f" % (z.mean(), 4.0 / math.sqrt(G), np.abs(z).max()))
    assert nref.same_estimand(z), z


# ---- 7. the scene's own camera -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cornell", "sphere-lamp"))
def test_render_nee_frame(name):
    """a 16 x 8 frame of the scene's own camera (pinhole: cornell; thin lens: sphere-lamp): the chunking changes no bit, and the frame is lit"""
    ctx, ds = _open(name)
    a = ds.render_nee(16, 8, 5, 5, depth=6, seed=11)
    b = ds.render_nee(16, 8, 5, 2, depth=6, seed=11)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    lin, rgb8, err, cnt = a
    assert lin.shape == (8, 16, 3) and rgb8.shape == (8, 16, 3) and err.shape == (8, 16) and cnt[1] == 16 * 8 * 5 and cnt[2] > cnt[3] > 0
    assert np.isfinite(lin).all() and (lin.sum(axis=2) > 0).mean() > 0.5
    assert not np.array_equal(ds.render_nee(16, 8, 5, 5, depth=6, seed=12)[0], lin)


def test_cli_nee_writes_the_light_sampled_frame(tmp_path, capsys):
    name = str(tmp_path / "box.ppm")
    assert core.main([name, "16", "8", "3", "cornell-box-classic", "--nee"]) == 0
    plain, lit = (tmp_path / "box.ppm").read_bytes(), (tmp_path / "box.nee.ppm").read_bytes()
    assert len(plain) == len(lit) and plain != lit and lit.startswith(b"P")


def test_render_with_nee_folds_a_generators_rays():
    """render_with(..., nee=True): a panorama of light-sampled paths; the chunking changes no bit, the paths are the plain frame's paths"""
    ctx, ds = _open("sphere-lamp")
    view = dict(lookfrom=(6.0, 3.0, 9.0), lookat=(0.0, 1.0, 0.0), vup=(0.0, 1.0, 0.0))
    a = ds.render_with(camera.panorama_rays, 16, 8, 5, 5, depth=6, nee=True, **view)
    b = ds.render_with(camera.panorama_rays, 16, 8, 5, 2, depth=6, nee=True, **view)
    plain = ds.render_with(camera.panorama_rays, 16, 8, 5, 5, depth=6, **view)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(a[3]) == 4 and a[3][:2].tolist() == plain[3].tolist() and a[3][2] > 0 and a[3][2] >= a[3][3] and not np.array_equal(a[0], plain[0])
