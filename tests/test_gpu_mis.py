"""Multiple importance sampling for the light-sampled paths on the device (rtmi_render_rays_mis*, rtmi_probe_paths_mis).  The probe's log must equal
rtmi_probe_paths' on the path itself, rtmi_probe_paths_nee's on light, ray and weight under the uniform pick, camera.mis_pick / nee_samples under
either, rtmi_query_occluded_device and the oracle on the shadow flags, and the MIS rule restated in numpy (tests/mis_reference.py) on x, m, g, x', the
contributions, the closing weight and the radiance -- all as exact doubles; every contribution must be at most T * Le; the render must equal the
probe; chunks, passes and the neighbouring cases must change no bit; and the estimate must have the plain path tracer's expectation."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from raytrace_clj_amd import _ffi, camera, core
from tests import direct_cases as dcs
from tests import direct_reference as dref
from tests import mis_cases as mcs
from tests import mis_reference as mref
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
    """one render_rays_device / render_rays_mis_device call on HBM buffers -> (mean, stderr, counters, radiance or None, state or None) on the host"""
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


def _check_log(f, what, precision, ds, rays, keys, depth, lights, choice, oracle_flags=True):
    """rtmi_probe_paths_mis against the device's own parts and the rule's restatement -> (radiance, the samples' dict with the log's states, weighted, weight)"""
    table = camera.light_table(f, lights)
    max_seg = depth + 1
    what = "%s %s depth %d choice %d" % (what, precision, depth, choice)
    rgb0, nseg0, log0, nlog0 = ds.probe_paths(rays, keys, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)
    rgb, nseg, log, nlog, weight = ds.probe_paths_mis(rays, keys, lights=lights, light_choice=choice, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)
    assert log.shape == (len(rays), max_seg, _ffi.MIS_REC)
    # the path itself is the plain path
    assert np.array_equal(bits(log[:, :, :12]), bits(log0)), what
    assert np.array_equal(nseg, nseg0) and np.array_equal(nlog, nlog0), what
    # step 1: where; steps 2 - 3: which light, the ray, w
    at = nref.vertices(f, log, nlog)
    assert np.array_equal(log[:, :, 12] != 0.0, at), what
    s = mref.samples(log, at, keys, table, choice)
    i, j, l, built = s["i"], s["j"], s["l"], s["built"]
    assert np.array_equal(log[i, j, 13], l.astype(np.float64)), what
    assert np.array_equal(bits(log[i, j, 14:17]), bits(s["d"])) and np.array_equal(bits(log[i, j, 17]), bits(s["w"])), what
    if choice == 0:  # l, d and w are the NEE probe's
        nee_log = ds.probe_paths_nee(rays, keys, lights=lights, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)[2]
        assert np.array_equal(bits(log[:, :, 13:18]), bits(nee_log[:, :, 13:18])) and np.array_equal(bits(log[:, :, 12]), bits(nee_log[:, :, 12])), what
    state = log[i, j, 12]
    assert np.array_equal(state == 3.0, ~built), what
    # the shadow flags are the any-hit query's on those rays, and the oracle's
    shadow = nref.shadow_rays(log, i, j, s["d"], rays[:, 6])[built]
    flags = _occluded(ds, shadow, precision)
    assert np.array_equal(state[built] == 2.0, flags == 1), what
    if oracle_flags and precision == "f64" and len(shadow):
        assert np.array_equal(_oracle().probe_hit(f, shadow, tmin=nref.T_MIN, tmax=nref.T_MAX)[:, 0] != 0.0, flags == 1), what
    # steps 4 and 6: x, m, g; T; step 5: the contributions, each at most T * Le, and their fold
    assert np.array_equal(bits(log[i, j, 24]), bits(s["x"])) and np.array_equal(bits(log[i, j, 25]), bits(s["m"])), what
    assert np.array_equal(bits(log[i, j, 26]), bits(s["g"])), what
    assert not log[:, :, 24:27][~at].any(), what
    T = nref.attenuations(f, log, nlog, np.float32 if precision == "f32" else np.float64)
    assert np.array_equal(bits(log[i, j, 18:21]), bits(T[i, j])), what
    contrib, accum = mref.fold(len(rays), max_seg, s, state == 1.0, T, table)
    assert np.array_equal(bits(log[:, :, 21:24]), bits(contrib)), what
    assert (log[i, j, 21:24] <= log[i, j, 18:21] * table[l, 7:10]).all() and (log[:, :, 21:24] >= 0.0).all(), what
    # step 7: which closing emissions are weighted, x', the factor, the radiance
    weighted, xq, mq = mref.closing(log, nlog, nseg, at, lights, s, table)
    want_xq = np.zeros(log.shape[:2])
    want_xq[np.flatnonzero(weighted), nlog[weighted] - 1] = xq[weighted]
    assert np.array_equal(bits(log[:, :, 27]), bits(want_xq)), what
    assert np.array_equal(bits(weight), bits(mq)) and (weight >= 0.0).all() and (weight <= 1.0).all() and (weight[~weighted] == 1.0).all(), what
    assert np.array_equal(bits(rgb), bits(accum + rgb0 * mq[:, None])), what
    s.update(state=state, weighted=weighted, weight=weight, nseg=nseg, log=log, nlog=nlog)
    return rgb, s


# ---- 1. the probe's log --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", mcs.CHOICES)
@pytest.mark.parametrize("name,precision", mcs.CASES)
def test_probe_log(name, precision, choice):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    f = dcs.flat(name)
    lights = dref.eligible(f)
    assert ds.lights().tolist() == lights.tolist() and len(lights) >= 1
    seen = set()
    for depth in mcs.DEPTHS:
        rgb, s = _check_log(f, name, precision, ds, rays, keys, depth, lights, choice)
        if depth == 0:
            assert len(s["state"]) == 0 and (s["nseg"] <= 1).all() and (s["weight"] == 1.0).all()  # no scatter, no light sample: the closing emission alone
        else:
            seen |= set(s["state"].tolist())
            assert s["weighted"].any() and not s["weighted"].all() and (s["weight"][s["weighted"]] < 1.0).any() and (s["weight"][s["weighted"]] > 0.0).any()
            assert (s["g"] > 0.0).any() and (s["x"] > 0.0).any()
    assert {1.0, 2.0, 3.0} <= seen  # unoccluded, occluded and unbuilt samples all occur


# ---- 2. the render against the probe, chunks and passes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", mcs.CHOICES)
@pytest.mark.parametrize("name,precision", mcs.CASES)
def test_render_equals_probe(name, precision, choice):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    lights = dref.eligible(dcs.flat(name))
    for depth in (3, 50):
        rgb, nseg, log, nlog, _ = ds.probe_paths_mis(rays, keys, light_choice=choice, depth=depth, ctr0=2, max_seg=depth + 1, precision=precision)
        state = log[:, :, 12]
        want = [int(nseg.sum()), N, int(((state == 1.0) | (state == 2.0)).sum()), int((state == 2.0).sum())]
        mean, se, cnt, out, _ = _device_render(ds, "render_rays_mis_device", N // 4, 4, rays, keys, light_choice=choice, ctr0=2, depth=depth, precision=precision)
        assert np.array_equal(bits(out), bits(rgb)) and cnt == want and want[2] > want[3] > 0, (name, precision, depth, cnt, want)
        h_mean, h_se, h_cnt, h_out = ds.render_rays_mis(rays, 4, lights=lights, light_choice=("uniform", "power")[choice], keys=keys, ctr0=2, depth=depth,
                                                        precision=precision, return_rays=True)
        assert np.array_equal(bits(h_out), bits(rgb)) and h_cnt.tolist() == want
        assert np.array_equal(bits(h_mean), bits(mean)) and np.array_equal(bits(h_se), bits(se))


@pytest.mark.parametrize("name,precision", mcs.CASES)
def test_chunks_give_the_bits_of_one_call(name, precision):
    ctx, ds = _open(name)
    ng, group = 60, 25
    rays = _inputs(name)[0].reshape(ng, group, 7)
    whole = np.zeros((ng, _ffi.RAYS_REC))
    one = _device_render(ds, "render_rays_mis_device", ng, group, rays.reshape(-1, 7), light_choice=1, seed=99, depth=8, precision=precision, first=0, state=whole)
    state, total, first = np.zeros((ng, _ffi.RAYS_REC)), np.zeros(4, np.int64), 0
    for size in (1, 7, group - 8):
        part = _device_render(ds, "render_rays_mis_device", ng, size, np.ascontiguousarray(rays[:, first:first + size]).reshape(-1, 7), light_choice=1, seed=99,
                              depth=8, precision=precision, first=first, state=state)
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
            outs.append(_device_render(ds, "render_rays_mis_device", ng, group, rays, seed=5, ctr0=2, depth=6, first=3, want_rays=False)[:3])
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1])) and outs[0][2] == outs[1][2]
    assert outs[0][2][1] == ng * group and outs[0][2][2] > 0


def test_the_estimate_differs_from_nee_and_from_the_plain_path():
    """the same paths (segments, rays, shadow rays), another estimate: the MIS call is neither of its neighbours"""
    ctx, ds = _open("cornell")
    rays, keys = _inputs("cornell")
    plain = _device_render(ds, "render_rays_device", N, 1, rays, keys, n_counters=2, ctr0=2, depth=50)
    nee = _device_render(ds, "render_rays_nee_device", N, 1, rays, keys, ctr0=2, depth=50)
    mis = _device_render(ds, "render_rays_mis_device", N, 1, rays, keys, ctr0=2, depth=50)
    assert mis[2] == nee[2] and mis[2][:2] == plain[2]
    assert not np.array_equal(bits(mis[3]), bits(nee[3])) and not np.array_equal(bits(mis[3]), bits(plain[3]))


# ---- 3. the light-list cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", mcs.CASES)
def test_no_lights_is_render_rays(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    plain = _device_render(ds, "render_rays_device", N // 4, 4, rays, keys, n_counters=2, ctr0=2, depth=50, precision=precision)
    for choice in mcs.CHOICES:
        none = _device_render(ds, "render_rays_mis_device", N // 4, 4, rays, keys, lights=[], light_choice=choice, ctr0=2, depth=50, precision=precision)
        assert all(np.array_equal(bits(none[k]), bits(plain[k])) for k in (0, 1, 3)) and none[2] == plain[2] + [0, 0]
    rgb, nseg, log, nlog, weight = ds.probe_paths_mis(rays, keys, lights=[], depth=50, ctr0=2, max_seg=4, precision=precision)
    assert np.array_equal(bits(rgb), bits(plain[3])) and (weight == 1.0).all() and not log[:, :, 12:].any()


def test_a_scene_without_eligible_lights_is_render_rays():
    ctx = core.Context(0)
    ds = core.DeviceScene(dcs.not_lights()["moving"], ctx=ctx)  # its lamp moves: it shines, but it is no light for these calls
    rays, keys = _inputs("sphere-lamp")
    assert len(ds.lights()) == 0
    plain = _device_render(ds, "render_rays_device", N, 1, rays, keys, n_counters=2, ctr0=2, depth=50)
    none = _device_render(ds, "render_rays_mis_device", N, 1, rays, keys, light_choice=1, ctr0=2, depth=50)
    assert all(np.array_equal(bits(none[k]), bits(plain[k])) for k in (0, 1, 3)) and none[2] == plain[2] + [0, 0] and plain[3].any()
    ds.close(); ctx.close()


def test_a_listed_subset_keeps_the_unlisted_lamp_whole():
    name = "example-light"
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    f = dcs.flat(name)
    both = dref.eligible(f)
    assert len(both) == 2
    all_weighted = _check_log(f, name, "f64", ds, rays, keys, 50, both, 1)[1]["weighted"]
    for listed in (both[:1], both[1:]):
        rgb, s = _check_log(f, name, "f64", ds, rays, keys, 50, listed, 1)  # (the restatement compares with the listed lamp alone)
        other = all_weighted & ~s["weighted"]  # paths that end on the unlisted lamp behind a light sample
        assert s["weighted"].any() and other.any() and (s["weight"][other] == 1.0).all() and not (s["weighted"] & ~all_weighted).any()
        out = _device_render(ds, "render_rays_mis_device", N, 1, rays, keys, lights=listed, light_choice=1, ctr0=2, depth=50)[3]
        assert np.array_equal(bits(out), bits(rgb))


def test_a_lamp_switched_off_is_never_picked_by_power_and_keeps_weight_one():
    """a material edit sets the rectangle lamp's Le to zero: it stays an eligible light; the uniform pick still samples it and weighs paths that end on
    it, the pick by power never picks it and its (black) emission keeps the factor 1"""
    ctx = core.Context(0)
    lit, dark = mcs.two_lamp_flat(), mcs.two_lamp_flat((0.0, 0.0, 0.0))
    ds = core.DeviceScene(lit, ctx=ctx)
    rays, keys = _inputs("example-light")
    lights = dref.eligible(lit)
    assert len(lights) == 2 and ds.lights().tolist() == lights.tolist()
    before = _check_log(lit, "two lamps", "f64", ds, rays, keys, 50, lights, 1)[1]
    assert set(before["l"].tolist()) == {0, 1}
    ds.set_materials(dark)
    assert ds.lights().tolist() == lights.tolist()
    table = camera.light_table(dark, lights)
    off = int(np.flatnonzero(~table[:, 7:10].any(axis=1))[0])
    rgb, s = _check_log(dark, "one lamp off", "f64", ds, rays, keys, 50, lights, 1)
    assert len(s["l"]) and not (s["l"] == off).any() and s["live"].tolist() == [k != off for k in range(2)] and s["q"][1 - off] == 1.0
    ends = s["log"][np.arange(N), np.maximum(s["nlog"] - 1, 0), 0].astype(np.int64)
    on_off = (s["nlog"] == s["nseg"]) & (s["nlog"] >= 2) & (ends == lights[off])
    assert on_off.any() and (s["weight"][on_off] == 1.0).all() and s["weighted"].any() and not (s["weighted"] & on_off).any()
    uniform = _check_log(dark, "one lamp off", "f64", ds, rays, keys, 50, lights, 0)[1]
    assert (uniform["l"] == off).any() and (uniform["weighted"] & on_off).any()
    out = _device_render(ds, "render_rays_mis_device", N, 1, rays, keys, light_choice=1, ctr0=2, depth=50)[3]
    assert np.array_equal(bits(out), bits(rgb))
    ds.close(); ctx.close()


# ---- 4. errors and zero work -----------------------------------------------------------------------------------------------------------------------
def test_errors_and_zero_work():
    L = _ffi.lib()
    ctx = core.Context(0)
    smoke = core.DeviceScene(ncs.media_flat(), ctx=ctx)
    _, ds = _open("sphere-lamp")
    rays = np.ascontiguousarray(_inputs("sphere-lamp")[0][:8])
    mean, se, cnt = np.full((8, 3), -7.0), np.full(8, -7.0), np.full(4, 9, np.uint64)
    lamp = np.asarray(ds.lights(), np.int32)

    def call(scene, n_groups=8, group=1, g_first=0, depth=5, n_lights=0, prims=None, choice=0, precision=0, r=rays, m=mean):
        return L.rtmi_render_rays_mis(scene.handle, precision, n_groups, group, g_first, core.ptr(r), None, 1, 0, depth, n_lights, core.ptr(prims), choice, None,
                                      core.ptr(m), core.ptr(se), None, core.ptr(cnt))
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)
    # rtmi_render_rays' own errors come first, in their order, whatever the lights, the choice and the scene are
    assert call(smoke, n_groups=-1, n_lights=len(many), prims=many, choice=2) == -1
    assert call(smoke, group=0, choice=2) == -1 and call(smoke, g_first=-1) == -1 and call(smoke, depth=-1) == -1
    assert call(smoke, r=None, n_lights=len(many), prims=many) == -1 and call(smoke, m=None, choice=2) == -1
    assert call(smoke, precision=7, n_lights=len(many), prims=many, choice=2) == -1
    assert call(smoke, precision=1, choice=2) == -3                              # (RTMI_F32 on a mixed-kind scene, as rtmi_render_rays)
    # then the list's length, then the choice, then zero work and the media, then the list's entries
    assert call(smoke, n_lights=len(many), prims=many, choice=2) == -1 and b"n_lights" in L.rtmi_last_error()
    assert call(smoke, n_lights=-1, prims=many) == -1
    for bad in (2, -1, 7):
        assert call(smoke, choice=bad) == -1 and b"light_choice" in L.rtmi_last_error()
        assert call(smoke, n_groups=0, choice=bad) == -1 and call(ds, n_lights=1, prims=np.array([0], np.int32), choice=bad) == -1
        assert b"light_choice" in L.rtmi_last_error()
    assert call(smoke) == -3 and call(smoke, n_lights=1, prims=np.array([0], np.int32), choice=1) == -3
    assert b"ConstantMedium" in L.rtmi_last_error()
    assert call(ds, n_lights=1, prims=np.array([0], np.int32)) == -1 and call(ds, n_lights=1, prims=np.array([10 ** 6], np.int32), choice=1) == -1
    assert (mean == -7.0).all() and (se == -7.0).all() and (cnt == 9).all()         # a failed call writes nothing
    # zero work succeeds, on any scene, and writes nothing
    assert call(smoke, n_groups=0) == 0 and call(ds, n_groups=0, r=None, m=None, choice=1) == 0 and (cnt == 9).all()
    assert call(ds, n_lights=1, prims=lamp, choice=1) == 0 and cnt[1] == 8 and (mean != -7.0).all()
    # the probe refuses the same things, and the python layer raises
    for scene, kw, code in ((smoke, {}, -3), (ds, {"light_choice": 2}, -1)):
        with pytest.raises(core.RtmiError) as ei:
            scene.probe_paths_mis(rays, np.arange(8, dtype=np.uint64), **kw)
        assert ei.value.code == code
        with pytest.raises(core.RtmiError) as ei:
            scene.render_rays_mis(rays, **kw)
        assert ei.value.code == code
    smoke.close(); ctx.close()


# ---- 5. the same estimand, on the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("near", "under"))
def test_same_estimand_on_the_device(which):
    """test_mis_host.test_same_estimand's near sets, counts (G = 48, n = 4096) and conditions, with render_rays_device as the plain side, both choices"""
    ctx, ds = _open(ncs.ESTIMAND_SCENE)
    rays, keys = mcs.near_inputs(_oracle(), None if which == "near" else mcs.UNDER_SHARE)
    G, n = mcs.NEAR_G, mcs.NEAR_N
    plain = _device_render(ds, "render_rays_device", G, n, rays, keys, n_counters=2, depth=ncs.ESTIMAND_DEPTH)[3]
    for choice in mcs.CHOICES:
        mis = _device_render(ds, "render_rays_mis_device", G, n, rays, keys, light_choice=choice, depth=ncs.ESTIMAND_DEPTH)[3]
        z = nref.z_scores(plain.reshape(G, n, 3), mis.reshape(G, n, 3))
        print("%s, choice %d: z mean %.3f (bound %.3f), max |z| %.3f" % (which, choice, z.mean(), 4.0 / math.sqrt(G), np.abs(z).max()))
        assert nref.same_estimand(z), z
        assert mis.reshape(G, n, 3).sum(axis=2).var(axis=1).mean() < 0.5 * plain.reshape(G, n, 3).sum(axis=2).var(axis=1).mean()


# ---- 6. the scene's own camera, the generators, the command line -------------------------------------------------------------------------------------
def test_render_nee_with_mis_and_render_with():
    """a 16 x 8 frame of the scene's own camera and a panorama: the chunking changes no bit, the paths are the NEE frame's paths, the frame is another"""
    ctx, ds = _open("cornell")
    a = ds.render_nee(16, 8, 5, 5, depth=6, seed=11, mis=True, light_choice="power")
    b = ds.render_nee(16, 8, 5, 2, depth=6, seed=11, mis=True, light_choice=1)
    nee = ds.render_nee(16, 8, 5, 5, depth=6, seed=11)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[3].tolist() == nee[3].tolist() and not np.array_equal(a[0], nee[0]) and np.isfinite(a[0]).all() and (a[0].sum(axis=2) > 0).mean() > 0.5
    _, sl = _open("sphere-lamp")
    view = dict(lookfrom=(6.0, 3.0, 9.0), lookat=(0.0, 1.0, 0.0), vup=(0.0, 1.0, 0.0))
    p = sl.render_with(camera.panorama_rays, 16, 8, 5, 5, depth=6, nee="mis", **view)
    q = sl.render_with(camera.panorama_rays, 16, 8, 5, 2, depth=6, nee="mis", light_choice=0, **view)
    lit = sl.render_with(camera.panorama_rays, 16, 8, 5, 5, depth=6, nee=True, **view)
    assert all(np.array_equal(x, y) for x, y in zip(p, q)) and p[3].tolist() == lit[3].tolist() and not np.array_equal(p[0], lit[0])
    with pytest.raises(ValueError):
        sl.render_with(camera.panorama_rays, 16, 8, 5, 5, nee="bdpt", **view)


def test_cli_mis_writes_the_frame(tmp_path):
    name = str(tmp_path / "box.ppm")
    assert core.main([name, "16", "8", "3", "cornell-box-classic", "--nee", "--mis", "power"]) == 0
    plain, nee, mis = ((tmp_path / n).read_bytes() for n in ("box.ppm", "box.nee.ppm", "box.mis.ppm"))
    assert len(plain) == len(mis) and plain != mis and nee != mis and mis.startswith(b"P")
