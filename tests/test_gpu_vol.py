"""Light-sampled paths and frames through participating media on the device (rtmi_render_rays_vol*, rtmi_probe_paths_vol, rtmi_render_lit_vol*).
Without media every output must be the NEE or MIS sibling's bit for bit.  With media the probe's log must equal rtmi_probe_paths' on the path itself,
the volume rule restated in numpy (tests/vol_reference.py) on light, ray, weight, x, m, g, the contributions, the closing weight and the radiance, and
rtmi_query_occluded with the shadow rays' own keys on the shadow flags -- all as exact doubles; the render must equal the probe; chunks, passes, the
camera source and the device form must change no bit; and the estimate must have the plain path tracer's expectation where two wrong rules do not.
The device is compared with itself and with numpy, not with the oracle: a free-flight distance goes through log (ocml against glibc)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lit_cases as lc
import rays_reference as rr
from raytrace_clj_amd import _ffi, camera, core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd import util
from tests import depth_cases as dc
from tests import direct_cases as dcs
from tests import direct_reference as dref
from tests import nee_cases as ncs
from tests import nee_reference as nref
from tests import vol_cases as vcs
from tests import vol_reference as vref

N = dcs.N_POINTS
bits = nref.bits
SEED = lc.SEED
E_ARG, E_UNSUPPORTED = -1, -3


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


@functools.lru_cache(maxsize=None)
def _ctx():
    return core.Context(0)


@functools.lru_cache(maxsize=None)
def _open(family, name):
    """one device scene per recipe for the whole module: "dcs" direct_cases' scenes (no media), "vcs" the media scenes"""
    return core.DeviceScene((dcs.flat if family == "dcs" else vcs.flat)(name), ctx=_ctx())


def _dev():
    import torch
    return torch.device("cuda", 0)


def _device_render(ds, call, n_groups, group, rays, keys=None, n_counters=4, state=None, want_rays=True, **kw):
    """one render_rays*_device call on HBM buffers -> (mean, stderr, counters, radiance or None, state or None) on the host"""
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


def _lit_call(ds, call, nx, ny, s_first, s_count, state=None, want_rays=True, want_camera=False, stream=None, **kw):
    """one render_lit_device / render_lit_vol_device call into poison-filled HBM buffers -> dict of host arrays"""
    import torch
    n = nx * ny * s_count
    full = lambda shape, v, dt=torch.float64: torch.full(shape, v, dtype=dt, device=_dev())
    d = dict(lin=full((ny, nx, 3), -7.0), se=full((ny, nx), -7.0), q=full((ny, nx, 3), 99, torch.uint8), cnt=full((4,), 9, torch.int64),
             rays=full((n, 3), -7.0) if want_rays else None, cam=full((n, 8), -7.0) if want_camera else None,
             state=torch.from_numpy(state).to(_dev()) if state is not None else None)
    torch.cuda.synchronize(_dev())
    getattr(ds, call)(nx, ny, s_first, s_count, d["lin"], d["se"], out_rgb8=d["q"], state=d["state"], out_rays=d["rays"], out_camera=d["cam"],
                      out_counters=d["cnt"], stream=stream, **kw)
    torch.cuda.synchronize(_dev())
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


# ---- 5. without media the calls are their siblings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_without_media_the_probe_is_the_siblings(name, precision):
    ds = _open("dcs", name)
    rays, keys = dcs.view_rays(_oracle(), name), ncs.path_keys()
    for depth in vcs.DEPTHS:
        kw = dict(depth=depth, ctr0=2, max_seg=depth + 1, precision=precision)
        rgb, nseg, log, nlog, dropped = ds.probe_paths_nee(rays, keys, **kw)
        v = ds.probe_paths_vol(rays, keys, estimator="nee", light_choice=1, **kw)  # (the NEE rule does not look at the choice)
        assert v[2].shape == (N, depth + 1, _ffi.VOL_REC)
        assert np.array_equal(bits(v[0]), bits(rgb)) and np.array_equal(v[1], nseg) and np.array_equal(v[3], nlog), (name, precision, depth)
        assert np.array_equal(bits(v[2][:, :, :24]), bits(log)) and not v[2][:, :, 24:].any()
        assert np.array_equal(v[4], np.where(dropped == 1, 0.0, 1.0)) and ((depth > 0) == bool(dropped.any()))
        for choice in (0, 1):
            rgb, nseg, log, nlog, weight = ds.probe_paths_mis(rays, keys, light_choice=choice, **kw)
            v = ds.probe_paths_vol(rays, keys, estimator=2, light_choice=choice, **kw)
            assert np.array_equal(bits(v[0]), bits(rgb)) and np.array_equal(v[1], nseg) and np.array_equal(v[3], nlog), (name, precision, depth, choice)
            assert np.array_equal(bits(v[2][:, :, :28]), bits(log)) and not v[2][:, :, 28].any() and np.array_equal(bits(v[4]), bits(weight))


@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_without_media_the_render_is_the_siblings(name, precision):
    ds = _open("dcs", name)
    rays, keys = dcs.view_rays(_oracle(), name), ncs.path_keys()
    ng, group = N // 4, 4
    for depth in vcs.DEPTHS:
        for estimator, choice, sibling, extra in ((1, 1, "render_rays_nee_device", {}), (2, 0, "render_rays_mis_device", {"light_choice": 0}),
                                                  (2, 1, "render_rays_mis_device", {"light_choice": 1})):
            kw = dict(ctr0=2, depth=depth, precision=precision, first=0)
            want = _device_render(ds, sibling, ng, group, rays, keys, state=np.zeros((ng, _ffi.RAYS_REC)), **kw, **extra)
            got = _device_render(ds, "render_rays_vol_device", ng, group, rays, keys, state=np.zeros((ng, _ffi.RAYS_REC)), estimator=estimator,
                                 light_choice=choice, **kw)
            assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in (0, 1, 3, 4)) and got[2] == want[2], (name, precision, depth, estimator, choice)
    host = ds.render_rays_vol(rays, group, estimator="mis", light_choice="power", keys=keys, ctr0=2, depth=50, precision=precision, return_rays=True)
    assert np.array_equal(bits(host[3]), bits(got[3])) and np.array_equal(bits(host[0]), bits(got[0])) and host[2].tolist() == got[2]


@pytest.mark.parametrize("name,precision", ncs.CASES)
def test_without_media_the_frame_is_render_lit(name, precision):
    ds = _open("dcs", name)
    nx, ny, ns = vcs.SHAPES[0]
    for depth in vcs.DEPTHS:
        for estimator, choice in vcs.ESTIMATORS:
            kw = dict(light_choice=choice, depth=depth, seed=SEED, precision=precision, want_camera=True)
            want = _lit_call(ds, "render_lit_device", nx, ny, 0, ns, estimator=estimator, **kw)
            got = _lit_call(ds, "render_lit_vol_device", nx, ny, 0, ns, estimator=estimator, **kw)
            for k in ("lin", "se", "q", "cnt", "rays", "cam"):
                assert np.array_equal(got[k], want[k]) and (got[k].dtype != np.float64 or np.array_equal(bits(got[k]), bits(want[k]))), (name, depth, estimator, k)


# ---- 6. the probe's log on the media scenes -------------------------------------------------------------------------------------------------------------
def _attenuations(f, log, nlog, s):
    """T behind every vertex: restated where every albedo is a Constant texture (the smoke box); the log's own elsewhere (textures are pinned elsewhere)"""
    try:
        return nref.attenuations(f, log, nlog), True
    except AssertionError:
        T = np.zeros(log.shape[:2] + (3,))
        T[s["i"], s["j"]] = log[s["i"], s["j"], 18:21]
        return T, False


def _check_log(f, what, ds, rays, keys, depth, lights, estimator, choice, ctr0=2):
    """rtmi_probe_paths_vol against the device's own parts and the rule's restatement -> (radiance, the samples' dict with the log's states and more)"""
    table = camera.light_table(f, lights)
    max_seg = depth + 1
    what = "%s depth %d estimator %d choice %d" % (what, depth, estimator, choice)
    rgb0, nseg0, log0, nlog0 = ds.probe_paths(rays, keys, depth=depth, ctr0=ctr0, max_seg=max_seg)
    rgb, nseg, log, nlog, weight = ds.probe_paths_vol(rays, keys, estimator=estimator, lights=lights, light_choice=choice, depth=depth, ctr0=ctr0,
                                                      max_seg=max_seg)
    assert log.shape == (len(rays), max_seg, _ffi.VOL_REC)
    # the path's own stream is untouched
    assert np.array_equal(bits(log[:, :, :12]), bits(log0)) and np.array_equal(nseg, nseg0) and np.array_equal(nlog, nlog0), what
    # step 1: exactly the scattered Lambertian and Isotropic vertices; column 28 is the material table's
    at, iso = vref.vertices(f, log, nlog)
    assert np.array_equal(log[:, :, 12] != 0.0, at) and np.array_equal(log[:, :, 28] == 1.0, iso) and not log[:, :, 28][~iso].any(), what
    # steps 2, 3, 5: l, d, w, x, m, g
    s = vref.samples(log, at, iso, keys, table, estimator, choice)
    i, j, built = s["i"], s["j"], s["built"]
    assert np.array_equal(log[i, j, 13], s["l"].astype(np.float64)), what
    assert np.array_equal(bits(log[i, j, 14:17]), bits(s["d"])) and np.array_equal(bits(log[i, j, 17]), bits(s["w"])), what
    for col, key in ((24, "x"), (25, "m"), (26, "g")):
        assert np.array_equal(bits(log[i, j, col]), bits(s[key])), (what, key)
    assert not log[:, :, 24:27][~at].any(), what
    state = log[i, j, 12]
    assert np.array_equal(state == 3.0, ~built), what
    # step 4: the shadow flags are the any-hit query's on those rays with their own keys from draw 0
    shadow = vref.shadow_rays(log, s, vref.times(log, iso, rays[:, 6]))[built]
    skeys = s["key"][built]
    flags = np.zeros(0, np.uint8)
    if len(shadow):
        flags = ds.occluded(shadow, t_range=np.tile([nref.T_MIN, nref.T_MAX], (len(shadow), 1)), keys=skeys, ctr0=0)[0].ravel()
    assert np.array_equal(state[built] == 2.0, flags == 1), (what, int(((state[built] == 2.0) != (flags == 1)).sum()))
    # the contributions, their fold, the closing emission and the radiance
    T, restated = _attenuations(f, log, nlog, s)
    assert np.array_equal(bits(log[i, j, 18:21]), bits(T[i, j])), what
    contrib, accum = vref.fold(len(rays), max_seg, s, state == 1.0, T, table, estimator)
    assert np.array_equal(bits(log[:, :, 21:24]), bits(contrib)), what
    weighted, xq, mq = vref.closing(log, nlog, nseg, at, lights, s, table, estimator)
    want_xq = np.zeros(log.shape[:2])
    want_xq[np.flatnonzero(weighted), nlog[weighted] - 1] = xq[weighted]
    assert np.array_equal(bits(log[:, :, 27]), bits(want_xq)), what
    assert np.array_equal(bits(weight), bits(mq)) and (weight >= 0.0).all() and (weight <= 1.0).all() and (weight[~weighted] == 1.0).all(), what
    assert np.array_equal(bits(rgb), bits(accum + rgb0 * mq[:, None])), what
    s.update(state=state, weighted=weighted, weight=weight, nseg=nseg, log=log, nlog=nlog, shadow=shadow, skeys=skeys, flags=flags, at=at, iso_at=iso,
             restated=restated)
    return rgb, s


@pytest.mark.parametrize("estimator,choice", vcs.ESTIMATORS)
@pytest.mark.parametrize("name", vcs.MEDIA_SCENES)
def test_probe_log_on_media(name, estimator, choice):
    ds = _open("vcs", name)
    f = vcs.flat(name)
    rays, keys = vcs.view_rays(_oracle(), name), ncs.path_keys()
    lights = dref.eligible(f)
    assert ds.lights().tolist() == lights.tolist() and len(lights) >= 1
    seen = set()
    for depth in vcs.DEPTHS:
        rgb, s = _check_log(f, name, ds, rays, keys, depth, lights, estimator, choice)
        if depth == 0:
            assert len(s["state"]) == 0 and (s["weight"] == 1.0).all()
            continue
        seen |= set(s["state"].tolist())
        if depth < 3:  # (a camera ray of the subsurface sphere reaches its medium through the glass: no Isotropic scatter with one bounce)
            continue
        assert s["iso"].any() and (~s["iso"]).any() and s["built"][s["iso"]].any(), name
        if depth < 50:
            continue
        # the keys were exercised: some shadow rays are stopped by a medium, and the unkeyed query answers otherwise somewhere
        shadow, skeys = s["shadow"], s["skeys"]
        tr = np.tile([nref.T_MIN, nref.T_MAX], (len(shadow), 1))
        hits = ds.query_hits(shadow, t_range=tr, keys=skeys, ctr0=0)
        hits = hits[0] if isinstance(hits, tuple) else hits
        prim = hits[hits[:, 0] != 0.0, 1].astype(np.int64)
        assert ((np.asarray(f.prim_kind)[prim] & 15) == fl.PRIM_MEDIUM).any(), name
        unkeyed = ds.occluded(shadow, t_range=tr)[0].ravel()
        if name == "subsurface":  # its one medium fills a glass ball: whatever the medium draws, the ball's own surface stops every ray that crosses it
            assert np.array_equal(unkeyed, s["flags"]), name
        else:
            assert not np.array_equal(unkeyed, s["flags"]), name
        assert s["weighted"].any(), name
    assert {1.0, 2.0} <= seen
    assert (name == "smoke") == s["restated"]


# ---- 7. the render equals the probe per ray; chunks and passes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator,choice", vcs.ESTIMATORS)
@pytest.mark.parametrize("name", vcs.MEDIA_SCENES)
def test_render_equals_probe(name, estimator, choice):
    ds = _open("vcs", name)
    rays, keys = vcs.view_rays(_oracle(), name), ncs.path_keys()
    for depth in (3, 50):
        rgb, nseg, log, nlog, _ = ds.probe_paths_vol(rays, keys, estimator=estimator, light_choice=choice, depth=depth, ctr0=2, max_seg=depth + 1)
        state = log[:, :, 12]
        want = [int(nseg.sum()), N, int(((state == 1.0) | (state == 2.0)).sum()), int((state == 2.0).sum())]
        mean, se, cnt, out, _ = _device_render(ds, "render_rays_vol_device", N // 4, 4, rays, keys, estimator=estimator, light_choice=choice, ctr0=2,
                                               depth=depth)
        assert np.array_equal(bits(out), bits(rgb)) and cnt == want and want[2] > want[3] > 0, (name, depth, cnt, want)
        emean, ese = rr.fold(rgb, 4, "f64")
        assert np.array_equal(bits(mean), bits(emean)) and np.array_equal(bits(se), bits(ese))
        h_mean, h_se, h_cnt, h_out = ds.render_rays_vol(rays, 4, estimator=estimator, light_choice=choice, keys=keys, ctr0=2, depth=depth, return_rays=True)
        assert np.array_equal(bits(h_out), bits(rgb)) and h_cnt.tolist() == want and np.array_equal(bits(h_mean), bits(mean))


@pytest.mark.parametrize("name", ("smoke", "final"))
def test_chunks_give_the_bits_of_one_call(name):
    ds = _open("vcs", name)
    ng, group = 500, 3
    rays = vcs.view_rays(_oracle(), name).reshape(ng, group, 7)
    kw = dict(estimator=2, light_choice=1, seed=99, depth=8)
    one = _device_render(ds, "render_rays_vol_device", ng, group, rays.reshape(-1, 7), first=0, state=np.zeros((ng, _ffi.RAYS_REC)), **kw)
    a = _device_render(ds, "render_rays_vol_device", ng, 2, np.ascontiguousarray(rays[:, 0:2]).reshape(-1, 7), first=0, state=np.zeros((ng, _ffi.RAYS_REC)), **kw)
    b = _device_render(ds, "render_rays_vol_device", ng, 1, np.ascontiguousarray(rays[:, 2:3]).reshape(-1, 7), first=2, state=a[4], **kw)
    assert np.array_equal(bits(b[0]), bits(one[0])) and np.array_equal(bits(b[1]), bits(one[1])) and np.array_equal(bits(b[4]), bits(one[4]))
    assert (np.array(a[2]) + np.array(b[2])).tolist() == one[2] and one[2][1] == ng * group and one[2][2] > one[2][3] > 0


def test_workspace_passes_inside_image_rows_change_no_bit():
    """without out_rays the radiance lives in the workspace: at its floor of 1 MiB a 40 x 24 x 100 frame (2.3 MB of samples) takes three passes of 436,
    436 and 88 pixels -- 436 = 10 rows and 36 pixels, so both boundaries fall inside an image row"""
    nx, ny, ns = 40, 24, 100
    per_pass = (1 << 20) // (ns * 24)
    assert -(-nx * ny // per_pass) >= 3 and per_pass % nx != 0 and (2 * per_pass) % nx != 0
    ds, ctx = _open("vcs", "smoke"), _ctx()
    outs = []
    try:
        for ws in (1 << 20, 64 << 30):
            ctx.set_option("workspace_bytes", ws)
            outs.append(_lit_call(ds, "render_lit_vol_device", nx, ny, 3, ns, want_rays=False, want_camera=True, estimator=2, depth=4, seed=SEED))
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
    for k in ("lin", "se", "q", "cam", "cnt"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(bits(outs[0]["lin"]), bits(outs[1]["lin"])) and outs[0]["cnt"][1] == nx * ny * ns and outs[0]["cnt"][2] > outs[0]["cnt"][3] > 0


# ---- 8. the frame ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vcs.SHAPES)
@pytest.mark.parametrize("name", ("smoke", "final"))
def test_every_row_of_the_frame_is_the_probes_path(name, shape):
    ds = _open("vcs", name)
    nx, ny, ns = shape
    keys = lc.frame_keys(nx, ny, ns, SEED)
    for depth in (3, 50) if shape == vcs.SHAPES[0] else (50,):
        for estimator, choice in vcs.ESTIMATORS:
            lin, q, err, cnt, out, cam = ds.render_lit_vol(nx, ny, ns, estimator=estimator, light_choice=choice, depth=depth, seed=SEED, return_rays=True,
                                                           return_camera=True)
            out, cam = out.reshape(-1, 3), cam.reshape(-1, 8)
            probe = lambda r, k, ctr0: ds.probe_paths_vol(r, k, estimator=estimator, light_choice=choice, depth=depth, ctr0=ctr0, max_seg=depth + 1)
            rgb, nseg, log, nlog, _ = lc.probe_by_ctr(probe, np.ascontiguousarray(cam[:, :7]), keys, cam[:, 7])
            w = (name, shape, depth, estimator, choice)
            assert np.array_equal(bits(out), bits(rgb)), (w, "%d of %d rows differ from the probe's" % ((bits(out) != bits(rgb)).any(axis=1).sum(), len(out)))
            state = log[:, :, 12]
            want = [int(nseg.sum()), nx * ny * ns, int(((state == 1.0) | (state == 2.0)).sum()), int((state == 2.0).sum())]
            assert cnt.tolist() == want and want[2] > want[3] > 0 and (log[:, :, 28] == 1.0).any(), (w, cnt, want)
            elin, eerr = lc.folded_frame(out, nx, ny, ns)
            assert np.array_equal(bits(lin), bits(elin)) and np.array_equal(bits(err), bits(eerr)), w
            assert np.array_equal(q, ds.ctx.denoise(lin, iterations=0)[1]), w
    # the paths are the plain frame's: the same segments, the same rays
    plain = ds.render_lit(nx, ny, ns, estimator="plain", depth=50, seed=SEED)
    assert plain[3].tolist()[:2] == cnt.tolist()[:2]
    chunked = ds.render_lit_vol(nx, ny, ns, chunk=1, estimator=estimator, light_choice=choice, depth=50, seed=SEED)
    assert np.array_equal(bits(chunked[0]), bits(lin)) and np.array_equal(chunked[1], q) and chunked[3].tolist() == cnt.tolist()


def test_a_moved_camera_is_the_fresh_scenes_view():
    import copy
    nx, ny, ns = vcs.SHAPES[0]
    f = vcs.flat("smoke")
    cam = np.array(f.cam, np.float64)
    assert int(f.cam_kind) == 1 and cam[21] == 0.0
    cam[21] = 0.3  # the scene's own thin lens opened to a real width
    g = copy.copy(f)
    g.cam_kind, g.cam = 1, cam
    moved, fresh = core.DeviceScene(f, ctx=_ctx()), core.DeviceScene(g, ctx=_ctx())
    kw = dict(estimator=2, light_choice=1, depth=6, seed=SEED, want_camera=True)
    try:
        before = _lit_call(moved, "render_lit_vol_device", nx, ny, 0, ns, **kw)
        want = _lit_call(fresh, "render_lit_vol_device", nx, ny, 0, ns, **kw)
        moved.set_camera((1, cam))
        got = _lit_call(moved, "render_lit_vol_device", nx, ny, 0, ns, **kw)
        for key in ("lin", "se", "q", "rays", "cam", "cnt"):
            assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(bits(got["rays"]), bits(want["rays"])) and not np.array_equal(bits(got["cam"]), bits(before["cam"]))
    finally:
        moved.close(); fresh.close()


def test_the_device_form_on_a_callers_stream_leaves_the_progressive_frame_alone():
    import torch
    nx, ny, ns = vcs.SHAPES[0]
    ds, ctx = _open("vcs", "smoke"), _ctx()
    kw = dict(estimator=2, depth=6, seed=SEED, want_camera=True)
    try:
        first = ds.render_progressive(nx, ny, 0, 2, 6, SEED, "f64")
        want = _lit_call(ds, "render_lit_vol_device", nx, ny, 0, ns, **kw)
        stream = torch.cuda.Stream(_dev())
        got = _lit_call(ds, "render_lit_vol_device", nx, ny, 0, ns, stream=stream.cuda_stream, **kw)
        for key in ("lin", "se", "q", "rays", "cam", "cnt"):
            assert np.array_equal(got[key], want[key]) and (got[key] != (99 if key == "q" else -7.0)).any(), key
        assert (got["cam"] != -7.0).all() and (got["rays"] != -7.0).all() and (got["se"] != -7.0).all()
        assert ctx.progressive_samples() == 2
        second = ds.render_progressive(nx, ny, 2, 1, 6, SEED, "f64")
        whole = ds.render(nx, ny, 3, 6, SEED, "f64")
        assert np.array_equal(bits(second[0]), bits(whole[0])) and not np.array_equal(bits(first[0]), bits(second[0]))
    finally:
        ctx.progressive_release()


# ---- 9. the same estimand, on the device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator,choice", vcs.ESTIMATORS[:2])
def test_same_estimand_on_the_device(estimator, choice):
    """test_vol_host.test_same_estimand's groups, counts and condition with render_rays_device as the plain side; the two controls are recomputed from
    the probe's logs: (a) on the floor groups the occluded light samples whose ray the box WITHOUT its media lets through are added back (media ignored
    by shadow rays); (b) on the smoke groups the closing emission behind an Isotropic light sample is added back whole (double counting)"""
    ds = _open("vcs", "smoke")
    f = vcs.flat("smoke")
    lights = dref.eligible(f)
    table = camera.light_table(f, lights)
    rays, keys, kind = vcs.estimand_inputs(_oracle())
    G, n, depth = vcs.ESTIMAND_G, vcs.ESTIMAND_N, vcs.ESTIMAND_DEPTH
    plain = _device_render(ds, "render_rays_device", G, n, rays, keys, n_counters=2, depth=depth)[3]
    vol = _device_render(ds, "render_rays_vol_device", G, n, rays, keys, estimator=estimator, light_choice=choice, depth=depth)[3]
    z = nref.z_scores(plain.reshape(G, n, 3), vol.reshape(G, n, 3))
    print("estimator %d: z mean %.3f (bound %.3f), max |z| %.3f" % (estimator, z.mean(), 4.0 / math.sqrt(G), np.abs(z).max()))
    assert nref.same_estimand(z), z
    rgb, nseg, log, nlog, weight = ds.probe_paths_vol(rays, keys, estimator=estimator, light_choice=choice, depth=depth, ctr0=0, max_seg=depth + 1)
    assert np.array_equal(bits(rgb), bits(vol))
    at, iso = vref.vertices(f, log, nlog)
    floor, smoke = np.repeat(kind == 1, n), np.repeat(kind == 0, n)
    # the white-smoke groups hold shadow rays that start inside a medium, both outcomes
    first = log[smoke, 0]
    assert (first[:, 28] == 1.0).mean() > 0.6 and (first[first[:, 28] == 1.0, 12] == 1.0).any() and (first[first[:, 28] == 1.0, 12] == 2.0).any()
    # (a) media ignored by the shadow rays
    s = vref.samples(log, at, iso, keys, table, estimator, choice)
    occluded = log[s["i"], s["j"], 12] == 2.0
    clear = core.DeviceScene(vcs.clear_flat(), ctx=_ctx())
    try:
        shadow = vref.shadow_rays(log, s, vref.times(log, iso, rays[:, 6]))[occluded]
        through = clear.occluded(shadow, t_range=np.tile([nref.T_MIN, nref.T_MAX], (len(shadow), 1)))[0].ravel() == 0
    finally:
        clear.close()
    T = nref.attenuations(f, log, nlog)
    back = np.zeros(len(s["i"]), bool)
    back[np.flatnonzero(occluded)[through]] = True
    extra, _ = vref.fold(len(rays), depth + 1, s, back, T, table, estimator)
    ignored = rgb + extra.sum(axis=1)
    za = nref.z_scores(plain[floor].reshape(-1, n, 3), ignored[floor].reshape(-1, n, 3))
    print("control, media ignored by shadow rays: mean %.3f, max |z| %.3f" % (za.mean(), np.abs(za).max()))
    assert through.any() and not nref.same_estimand(za)
    # (b) the closing emission kept whole behind an Isotropic light sample
    rows = np.arange(len(rays))
    behind_iso = (weight < 1.0) & iso[rows, np.maximum(nlog.astype(np.int64) - 2, 0)]
    twice = rgb + np.where(behind_iso[:, None], plain * (1.0 - weight)[:, None], 0.0)
    zb = nref.z_scores(plain[smoke].reshape(-1, n, 3), twice[smoke].reshape(-1, n, 3))
    print("control, closing emission kept behind an Isotropic sample: mean %.3f, max |z| %.3f" % (zb.mean(), np.abs(zb).max()))
    assert behind_iso[smoke].any() and not nref.same_estimand(zb)


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_in_order_and_the_siblings_still_refuse_media():
    L = _ffi.lib()
    smoke, ds = _open("vcs", "smoke"), _open("dcs", "sphere-lamp")
    hitlist = core.DeviceScene(dc.flat("hitlist-media"), ctx=_ctx())
    rays = np.ascontiguousarray(vcs.view_rays(_oracle(), "smoke")[:8])
    mean, se, cnt = np.full((8, 3), -7.0), np.full(8, -7.0), np.full(4, 9, np.uint64)
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)
    err = lambda: L.rtmi_last_error()

    def call(scene, n_groups=8, depth=5, estimator=2, n_lights=0, prims=None, choice=0, precision=0):
        return L.rtmi_render_rays_vol(scene.handle, precision, n_groups, 1, 0, core.ptr(rays), None, 1, 0, depth, estimator, n_lights, core.ptr(prims), choice,
                                      None, core.ptr(mean), core.ptr(se), None, core.ptr(cnt))

    def lit(scene, nx=2, ny=4, estimator=2, n_lights=0, prims=None, choice=0, precision=0):
        return L.rtmi_render_lit_vol(scene.handle, precision, nx, ny, 0, 1, 5, 1, estimator, n_lights, core.ptr(prims), choice, None, core.ptr(mean), None,
                                     core.ptr(se), None, None, core.ptr(cnt))

    def probe(scene, estimator=2, n_lights=0, prims=None, choice=0):
        return L.rtmi_probe_paths_vol(scene.handle, 0, 8, core.ptr(rays), core.ptr(np.arange(8, dtype=np.uint64)), 0, 5, estimator, n_lights, core.ptr(prims),
                                      choice, core.ptr(mean), None, None, None, 0, None)
    for fn in (call, lit, probe):
        # the sibling's own come first (RTMI_F32 on a mixed-kind scene among them), then the list's length, the estimator, the choice
        wrong = 0 if fn is lit else 9  # (rtmi_render_lit's own range check of 0..2 stands before its handle check: test_vol_host.py)
        if fn is not probe:
            assert fn(hitlist, precision=1, estimator=wrong, choice=5) == E_UNSUPPORTED and fn(hitlist, precision=7, estimator=wrong) == E_ARG
        assert fn(hitlist, n_lights=len(many), prims=many, estimator=wrong, choice=5) == E_ARG and b"n_lights" in err()
        for e in (0, 3, -1) if fn is not lit else (0,):
            assert fn(hitlist, estimator=e, choice=5) == E_ARG and b"estimator" in err(), (fn, e)
        assert fn(hitlist, estimator=2, choice=5) == E_ARG and b"light_choice" in err()
        assert fn(hitlist, estimator=1, choice=5) == E_UNSUPPORTED                   # the NEE rule does not look at the choice: the next error
        # media outside RTMI_MEDIA_DESCENT, before the list's entries
        assert fn(hitlist, n_lights=1, prims=np.array([10 ** 6], np.int32)) == E_UNSUPPORTED and b"RTMI_MEDIA_DESCENT" in err()
        assert fn(smoke, n_lights=1, prims=np.array([10 ** 6], np.int32)) == E_ARG and fn(smoke, n_lights=1, prims=np.array([0], np.int32)) == E_ARG
        assert (mean == -7.0).all() and (se == -7.0).all() and (cnt == 9).all()        # a failed call launches nothing and writes nothing
    assert call(hitlist, n_groups=0) == 0 and call(hitlist, n_groups=0, estimator=0) == E_ARG and call(hitlist, n_groups=0, choice=2) == E_ARG
    assert (cnt == 9).all()
    assert call(smoke) == 0 and cnt[1] == 8 and cnt[2] > 0 and (mean != -7.0).all()
    # the existing calls keep refusing the smoke box; the python layer raises
    keys = np.arange(8, dtype=np.uint64)
    for refused in (lambda: smoke.render_rays_nee(rays), lambda: smoke.render_rays_mis(rays), lambda: smoke.probe_paths_nee(rays, keys),
                    lambda: smoke.probe_paths_mis(rays, keys), lambda: smoke.render_lit(4, 2, 1, estimator="nee"), lambda: smoke.render_lit(4, 2, 1, estimator="mis"),
                    lambda: hitlist.render_rays_vol(rays), lambda: hitlist.render_lit_vol(4, 2, 1), lambda: hitlist.probe_paths_vol(rays, keys)):
        with pytest.raises(core.RtmiError) as ei:
            refused()
        assert ei.value.code == E_UNSUPPORTED
    with pytest.raises(core.RtmiError) as ei:
        smoke.render_lit_vol(4, 2, 1, estimator=0)
    assert ei.value.code == E_ARG
    assert smoke.render_lit(4, 2, 1, estimator="plain")[3][1] == 8  # (the plain estimator traces media, as before)
    hitlist.close()


# ---- the generators and the command line ------------------------------------------------------------------------------------------------------------------
def test_render_with_and_the_command_line(tmp_path):
    ds = _open("vcs", "smoke")
    view = dict(lookfrom=(278.0, 278.0, -100.0), lookat=(278.0, 278.0, 0.0), vup=(0.0, 1.0, 0.0))
    p = ds.render_with(camera.panorama_rays, 16, 8, 4, 4, depth=6, nee="vol-mis", light_choice=1, **view)
    q = ds.render_with(camera.panorama_rays, 16, 8, 4, 1, depth=6, nee="vol-mis", light_choice=1, **view)
    e = ds.render_with(camera.panorama_rays, 16, 8, 4, 4, depth=6, nee="vol-nee", **view)
    assert all(np.array_equal(x, y) for x, y in zip(p, q)) and p[3].tolist() == e[3].tolist() and not np.array_equal(p[0], e[0]) and p[3][2] > 0
    with pytest.raises(core.RtmiError):
        ds.render_with(camera.panorama_rays, 16, 8, 4, 4, depth=6, nee="mis", **view)
    name = str(tmp_path / "box.ppm")
    assert core.main([name, "16", "8", "3", "cornell-box", "--lit-vol", "mis:power", "--chunk", "2"]) == 0
    plain, vol = ((tmp_path / n).read_bytes() for n in ("box.ppm", "box.vol.ppm"))
    assert len(plain) == len(vol) and plain != vol and vol.startswith(b"P")
