"""The proposal rule on the device (rtmi_render_rays_ris*, rtmi_probe_paths_ris, rtmi_render_lit_ris*).  The probe's log must equal rtmi_probe_paths' on
the path itself and the rule restated in numpy (tests/ris_reference.py over camera.ris_candidates / ris_choose) on the chosen candidate, S, w^, r, the live
count, the contributions, the closing weight and the radiance -- all as exact doubles; every contribution must keep the rule's bound; the shadow flags
must be rtmi_query_occluded_device's and the oracle's; with one lamp everything must be the MIS rule's under the uniform pick; the render must equal the
probe, the frame the probe on its own camera rays; chunks, passes and tile lists must change no bit; and the estimate must have the plain path tracer's
expectation where its two wrong neighbours do not."""
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
from tests import ris_cases as rcs
from tests import ris_reference as rref

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
    return ctx, core.DeviceScene(rcs.flat(name), ctx=ctx)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _inputs(name):
    return rcs.view_rays(_oracle(), name), ncs.path_keys()


def _occluded(ds, rays, precision):
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


def _check_log(f, what, precision, ds, rays, keys, depth, lights, oracle_flags=True):
    """rtmi_probe_paths_ris against the device's own parts and the rule's restatement -> (radiance, the samples' dict with the log's states)"""
    table = camera.light_table(f, lights)
    max_seg = depth + 1
    what = "%s %s depth %d" % (what, precision, depth)
    rgb0, nseg0, log0, nlog0 = ds.probe_paths(rays, keys, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)
    rgb, nseg, log, nlog, weight = ds.probe_paths_ris(rays, keys, lights=lights, depth=depth, ctr0=2, max_seg=max_seg, precision=precision)
    assert log.shape == (len(rays), max_seg, _ffi.RIS_REC)
    # the path itself is the plain path
    assert np.array_equal(bits(log[:, :, :12]), bits(log0)), what
    assert np.array_equal(nseg, nseg0) and np.array_equal(nlog, nlog0), what
    # step 1: where; steps 2 - 3: the chosen candidate, its ray, w, x, m; S, w^, r, the live count
    at = nref.vertices(f, log, nlog)
    assert np.array_equal(log[:, :, 12] != 0.0, at), what
    s = rref.samples(log, at, keys, table)
    i, j, l, built = s["i"], s["j"], s["l"], s["built"]
    assert np.array_equal(log[i, j, 13], l.astype(np.float64)), what
    assert np.array_equal(bits(log[i, j, 14:17]), bits(s["d"])) and np.array_equal(bits(log[i, j, 17]), bits(s["w"])), what
    assert np.array_equal(bits(log[i, j, 24]), bits(s["x"])) and np.array_equal(bits(log[i, j, 25]), bits(s["m"])), what
    assert np.array_equal(bits(log[i, j, 26]), bits(s["g"])), what
    assert np.array_equal(bits(log[i, j, 28]), bits(s["S"])) and np.array_equal(bits(log[i, j, 29]), bits(s["what"])), what
    assert np.array_equal(bits(log[i, j, 30]), bits(s["r"])) and np.array_equal(log[i, j, 31], s["count"].astype(np.float64)), what
    assert not log[:, :, 24:27][~at].any() and not log[:, :, 28:32][~at].any(), what
    state = log[i, j, 12]
    assert np.array_equal(state == 3.0, ~built), what
    # the shadow flags are the any-hit query's on those rays, and the oracle's
    shadow = nref.shadow_rays(log, i, j, s["d"], rays[:, 6])[built]
    flags = _occluded(ds, shadow, precision)
    assert np.array_equal(state[built] == 2.0, flags == 1), what
    if oracle_flags and precision == "f64" and len(shadow):
        assert np.array_equal(_oracle().probe_hit(f, shadow, tmin=nref.T_MIN, tmax=nref.T_MAX)[:, 0] != 0.0, flags == 1), what
    # T; step 5: the contributions, each within the rule's bound, and their fold
    T = nref.attenuations(f, log, nlog, np.float32 if precision == "f32" else np.float64)
    assert np.array_equal(bits(log[i, j, 18:21]), bits(T[i, j])), what
    contrib, accum = rref.fold(len(rays), max_seg, s, state == 1.0, T, table)
    assert np.array_equal(bits(log[:, :, 21:24]), bits(contrib)), what
    assert (log[i, j, 21:24] <= rref.bound(s, T, table) * (1.0 + 2.0 ** -50)).all() and (log[:, :, 21:24] >= 0.0).all(), what
    # step 7: which closing emissions are weighted, x', the factor, the radiance
    weighted, xq, mq = rref.closing(log, nlog, nseg, at, lights, s, table)
    want_xq = np.zeros(log.shape[:2])
    want_xq[np.flatnonzero(weighted), nlog[weighted] - 1] = xq[weighted]
    assert np.array_equal(bits(log[:, :, 27]), bits(want_xq)), what
    assert np.array_equal(bits(weight), bits(mq)) and (weight >= 0.0).all() and (weight <= 1.0).all() and (weight[~weighted] == 1.0).all(), what
    assert np.array_equal(bits(rgb), bits(accum + rgb0 * mq[:, None])), what
    s.update(state=state, weighted=weighted, weight=weight, nseg=nseg, log=log, nlog=nlog)
    return rgb, s


# ---- 1. the probe's log against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", rcs.CASES + (("lamps32", "f64"),) + rcs.ONE_LAMP_CASES)
def test_probe_log(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    f = rcs.flat(name)
    lights = dref.eligible(f)
    assert ds.lights().tolist() == lights.tolist() and len(lights) >= 1
    seen, counts = set(), set()
    for depth in rcs.DEPTHS:
        rgb, s = _check_log(f, name, precision, ds, rays, keys, depth, lights)
        if depth == 0:
            assert len(s["state"]) == 0 and (s["nseg"] <= 1).all() and (s["weight"] == 1.0).all()
        else:
            seen |= set(s["state"].tolist())
            counts |= set(s["count"].tolist())
            assert s["weighted"].any() and (s["g"] > 0.0).any() and (s["r"][s["built"]] >= 1.0).all()
    assert {1.0, 2.0, 3.0} <= seen
    if name == "lamps32":  # every one of the 32 lamps is chosen somewhere, and some vertex weighs more than half of them
        assert max(counts) >= 17 and (s["r"] > 1.0).any() and set(s["l"][s["built"]].tolist()) == set(range(32)) and s["live"].all()
    elif (name, precision) in rcs.CASES:  # many lamps: the reservoir replaced a candidate somewhere, and the lamp switched off was never live
        assert max(counts) >= 3 and (s["r"] > 1.0).any() and len(set(s["l"][s["built"]].tolist())) >= 3
        off = np.flatnonzero(~s["live"])
        assert len(off) == 1 and not (s["l"][s["built"]] == off[0]).any()


# ---- 2. the one-lamp cases are the MIS rule's under the uniform pick --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", rcs.ONE_LAMP_CASES)
def test_one_lamp_is_the_mis_rule(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    lights = dref.eligible(rcs.flat(name))[:1]  # (example-light holds two: its first alone)
    for depth in (3, 50):
        kw = dict(lights=lights, depth=depth, ctr0=2, max_seg=depth + 1, precision=precision)
        rgb, nseg, log, nlog, weight = ds.probe_paths_ris(rays, keys, **kw)
        m_rgb, m_nseg, m_log, m_nlog, m_weight = ds.probe_paths_mis(rays, keys, light_choice=0, **kw)
        assert np.array_equal(bits(rgb), bits(m_rgb)) and np.array_equal(bits(weight), bits(m_weight)) and np.array_equal(nseg, m_nseg)
        same = np.ones(_ffi.MIS_REC, bool)
        same[12] = False
        assert np.array_equal(bits(log[:, :, :_ffi.MIS_REC][:, :, same]), bits(m_log[:, :, same]))
        exempt = (m_log[:, :, 12] != 0.0) & (m_log[:, :, 25] == 0.0)  # MIS built a ray whose share m is +0.0: no live candidate here
        assert np.array_equal(log[:, :, 12][~exempt], m_log[:, :, 12][~exempt])
        built = (log[:, :, 12] == 1.0) | (log[:, :, 12] == 2.0)
        assert built.any() and (log[:, :, 30][built] == 1.0).all() and (log[:, :, 31][built] == 1.0).all()


# ---- 3. the render against the probe, chunks and passes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", rcs.CASES + (("lamps32", "f64"),))
def test_render_equals_probe(name, precision):
    ctx, ds = _open(name)
    rays, keys = _inputs(name)
    lights = dref.eligible(rcs.flat(name))
    for depth in (3, 50):
        rgb, nseg, log, nlog, _ = ds.probe_paths_ris(rays, keys, depth=depth, ctr0=2, max_seg=depth + 1, precision=precision)
        state = log[:, :, 12]
        want = [int(nseg.sum()), N, int(((state == 1.0) | (state == 2.0)).sum()), int((state == 2.0).sum())]
        mean, se, cnt, out, _ = _device_render(ds, "render_rays_ris_device", N // 4, 4, rays, keys, ctr0=2, depth=depth, precision=precision)
        assert np.array_equal(bits(out), bits(rgb)) and cnt == want and want[2] > want[3] > 0, (name, precision, depth, cnt, want)
        h_mean, h_se, h_cnt, h_out = ds.render_rays_ris(rays, 4, lights=lights, keys=keys, ctr0=2, depth=depth, precision=precision, return_rays=True)
        assert np.array_equal(bits(h_out), bits(rgb)) and h_cnt.tolist() == want
        assert np.array_equal(bits(h_mean), bits(mean)) and np.array_equal(bits(h_se), bits(se))
        # mean and standard error are the fold of the rays' radiance: rtmi_render_rays' fold of the same rows
        state0 = np.zeros((N // 4, _ffi.RAYS_REC))
        one = _device_render(ds, "render_rays_ris_device", N // 4, 4, rays, keys, ctr0=2, depth=depth, precision=precision, first=0, state=state0)
        assert np.array_equal(bits(one[0]), bits(mean)) and np.array_equal(bits(one[1]), bits(se)) and (one[4][:, 9] == 4.0).all()
        # (the fold runs in the call's precision: four non-negative terms, three additions and a scaling on each side -- within 16 units of its rounding)
        eps = 2.0 ** -24 if precision == "f32" else 2.0 ** -53
        grouped = out.reshape(N // 4, 4, 3)
        assert np.allclose(mean, grouped.mean(axis=1), rtol=16 * eps, atol=0)
        # the standard error against an independent two-pass fold of the same rows (frame_reference.stderr_two_pass' formula: the largest channel's).
        # The device folds by Welford in the call's precision: its M2 is off by at most a few roundings of the largest squared sample, 8 eps x max^2
        # say, and sqrt(a + e) - sqrt(a) <= sqrt(e): an absolute sqrt(8 eps) x max |sample| per group, beside 16 roundings of the value itself.
        two_pass = np.sqrt(grouped.var(axis=1, ddof=1) / 4.0).max(axis=1)
        assert (np.abs(se - two_pass) <= 16 * eps * two_pass + math.sqrt(8 * eps) * np.abs(grouped).max(axis=(1, 2))).all() and (se > 0.0).any()
    if name == "lamps32":  # a 1-entry list runs too, and lamps32 chose among many
        assert len(lights) == 32 and log[:, :, 31].max() >= 8
        one = _device_render(ds, "render_rays_ris_device", N // 4, 4, rays, keys, lights=lights[5:6], ctr0=2, depth=3, precision=precision)
        mis = _device_render(ds, "render_rays_mis_device", N // 4, 4, rays, keys, lights=lights[5:6], light_choice=0, ctr0=2, depth=3, precision=precision)
        assert np.array_equal(bits(one[3]), bits(mis[3])) and one[2] == mis[2] and one[2][2] > 0


@pytest.mark.parametrize("name,precision", rcs.CASES)
def test_chunks_give_the_bits_of_one_call(name, precision):
    ctx, ds = _open(name)
    ng, group = 60, 25
    rays = _inputs(name)[0].reshape(ng, group, 7)
    whole = np.zeros((ng, _ffi.RAYS_REC))
    one = _device_render(ds, "render_rays_ris_device", ng, group, rays.reshape(-1, 7), seed=99, depth=8, precision=precision, first=0, state=whole)
    state, total, first = np.zeros((ng, _ffi.RAYS_REC)), np.zeros(4, np.int64), 0
    for size in (1, 7, group - 8):
        part = _device_render(ds, "render_rays_ris_device", ng, size, np.ascontiguousarray(rays[:, first:first + size]).reshape(-1, 7), seed=99,
                              depth=8, precision=precision, first=first, state=state)
        state, first, total = part[4], first + size, total + np.array(part[2])
    assert first == group
    assert np.array_equal(bits(part[0]), bits(one[0])) and np.array_equal(bits(part[1]), bits(one[1])) and np.array_equal(bits(state), bits(one[4]))
    assert total.tolist() == [one[2][0], ng * group, one[2][2], one[2][3]] and one[2][1] == ng * group and one[2][2] > 0


def test_workspace_passes_change_no_bit():
    """without out_rays the radiance lives in the workspace: option workspace_bytes at its floor splits the call into passes of whole groups"""
    ctx, ds = _open("lamps8")
    ng, group = 9000, 7  # 63 000 rays x 24 bytes = 1.5 MB: two passes at 1 MiB
    rays = np.tile(_inputs("lamps8")[0], (42, 1))
    outs = []
    try:
        for ws in (1 << 20, 64 << 30):
            ctx.set_option("workspace_bytes", ws)
            outs.append(_device_render(ds, "render_rays_ris_device", ng, group, rays, seed=5, ctr0=2, depth=6, first=3, want_rays=False)[:3])
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1])) and outs[0][2] == outs[1][2]
    assert outs[0][2][1] == ng * group and outs[0][2][2] > 0


# ---- 4. the frame ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", rcs.FRAMES)
def test_the_frame(nx, ny):
    ctx, ds = _open("lamps8")
    ns, depth, seed = 3, 6, 77
    lin, q, err, cnt, rays, cam = ds.render_lit_ris(nx, ny, ns, depth=depth, seed=seed, return_rays=True, return_camera=True)
    m_cam = ds.render_lit(nx, ny, ns, estimator="mis", depth=depth, seed=seed, return_camera=True)[4]
    assert np.array_equal(bits(cam), bits(m_cam))
    # every row is the probe on that ray from that stream position
    x, y = np.arange(nx * ny) % nx, np.arange(nx * ny) // nx
    g, s = (a.ravel() for a in np.meshgrid((ny - 1 - y) * nx + x, np.arange(ns), indexing="ij"))
    from raytrace_clj_amd import util
    keys = util.sample_keys(seed, g, s)
    flat_cam = cam.reshape(-1, 8)
    rgb = np.zeros((len(keys), 3))
    for pos in np.unique(flat_cam[:, 7]):  # (a pinhole or fixed lens: one stream position; a thin lens: one per number of rounds)
        rows = np.flatnonzero(flat_cam[:, 7] == pos)
        rgb[rows] = ds.probe_paths_ris(flat_cam[rows, :7], keys[rows], depth=depth, ctr0=int(pos))[0]
    assert np.array_equal(bits(rays.reshape(-1, 3)), bits(rgb)) and cnt[1] == nx * ny * ns and cnt[2] > cnt[3] > 0
    # chunks through the state change no bit
    chunked = ds.render_lit_ris(nx, ny, ns, chunk=2, depth=depth, seed=seed)
    assert all(np.array_equal(a, b) for a, b in zip(chunked[:3], (lin, q, err))) and chunked[3].tolist() == cnt.tolist()
    # all tiles listed: the whole-frame call's result
    tx, ty = (nx + 7) // 8, (ny + 7) // 8
    l2, q2, e2 = np.full((ny, nx, 3), -7.0), np.full((ny, nx, 3), 9, np.uint8), np.full((ny, nx), -7.0)
    c2, r2, k2 = ds.render_lit_ris(nx, ny, ns, depth=depth, seed=seed, tiles=np.arange(tx * ty), linear=l2, rgb8=q2, stderr=e2, return_rays=True, return_camera=True)
    assert np.array_equal(bits(l2), bits(lin)) and np.array_equal(q2, q) and np.array_equal(bits(e2), bits(err)) and c2.tolist() == cnt.tolist()
    # a tile subset writes the listed pixels with the whole-frame call's bits and leaves every other element's bits alone
    sub = np.arange(tx * ty, dtype=np.int32)[1::2]  # (13 x 7: the partial tile of its two; 19 x 11: three of six)
    l3, q3, e3 = np.full((ny, nx, 3), -7.0), np.full((ny, nx, 3), 9, np.uint8), np.full((ny, nx), -7.0)
    ds.render_lit_ris(nx, ny, ns, depth=depth, seed=seed, tiles=sub, linear=l3, rgb8=q3, stderr=e3)
    inside = np.zeros((ny, nx), bool)
    for t in sub:
        inside[(t // tx) * 8:(t // tx) * 8 + 8, (t % tx) * 8:(t % tx) * 8 + 8] = True
    assert np.array_equal(bits(l3[inside]), bits(lin[inside])) and np.array_equal(q3[inside], q[inside]) and np.array_equal(bits(e3[inside]), bits(err[inside]))
    assert (l3[~inside] == -7.0).all() and (q3[~inside] == 9).all() and (e3[~inside] == -7.0).all() and inside.any() and not inside.all()
    # an empty list succeeds and writes nothing
    c4 = ds.render_lit_ris(nx, ny, ns, depth=depth, seed=seed, tiles=np.zeros(0, np.int32), linear=l3, rgb8=q3, stderr=e3)[0]
    assert (c4 == 0).all() and (l3[~inside] == -7.0).all()


def test_adaptive_ris_on_the_cornell_box():
    """two rounds: the tiles that retired after the first hold render_lit_ris with its samples, the others with both rounds'"""
    ctx, ds = _open("cornell")
    nx, ny, first, chunk = 19, 11, 4, 4
    eps = float(np.median(ds.render_lit_ris(nx, ny, first, depth=5)[2]))
    lin, q, err, smp, cnt, rounds = ds.refine_lit_adaptive(nx, ny, first + chunk, chunk, eps, first=first, estimator="ris", depth=5)
    assert len(rounds) == 2 and rounds[0][0] == first and 0 < len(rounds[0][1]) < ((nx + 7) // 8) * ((ny + 7) // 8)
    assert set(np.unique(smp).tolist()) == {first, first + chunk}
    for n in (first, first + chunk):
        one = ds.render_lit_ris(nx, ny, n, depth=5)
        took = smp == n
        assert np.array_equal(bits(lin[took]), bits(one[0][took])) and np.array_equal(q[took], one[1][took]) and np.array_equal(bits(err[took]), bits(one[2][took]))


# ---- 5. expectation ----------------------------------------------------------------------------------------------------------------------------------
def test_same_estimand_on_the_device():
    """ris_cases' near set of lamps8's floor, mis_cases' z-test with its own thresholds (G = 48, n = 4096, depth 3) against render_rays_device: the
    device's rule passes; its two wrong neighbours, built from the device's own log, fail"""
    ctx, ds = _open("lamps8")
    f = rcs.flat("lamps8")
    lights = dref.eligible(f)
    table = camera.light_table(f, lights)
    rays, keys = rcs.near_inputs(_oracle())
    G, n, depth = rcs.NEAR_G, rcs.NEAR_N, rcs.NEAR_DEPTH
    plain = _device_render(ds, "render_rays_device", G, n, rays, keys, n_counters=2, depth=depth)[3].reshape(G, n, 3)
    ris = _device_render(ds, "render_rays_ris_device", G, n, rays, keys, depth=depth)[3]
    z = nref.z_scores(plain, ris.reshape(G, n, 3))
    print("correct: z mean %.3f (bound %.3f), max |z| %.3f" % (z.mean(), 4.0 / math.sqrt(G), np.abs(z).max()))
    assert nref.same_estimand(z), z
    # control A drops r from the logged contributions; control B weighs the closing emission with q = nl
    rgb, nseg, log, nlog, weight = ds.probe_paths_ris(rays, keys, depth=depth, max_seg=depth + 1)
    assert np.array_equal(bits(rgb), bits(ris))
    rgb0 = ds.probe_paths(rays, keys, depth=depth, max_seg=depth + 1)[0]
    with np.errstate(all="ignore"):
        a_contrib = np.where(log[:, :, 30:31] > 0.0, log[:, :, 21:24] / log[:, :, 30:31], 0.0)
    control_a = a_contrib.sum(axis=1) + rgb0 * weight[:, None]
    at = nref.vertices(f, log, nlog)
    s = rref.samples(log, at, keys, table, control="B")
    mq_b = rref.closing(log, nlog, nseg, at, lights, s, table)[2]
    control_b = (rgb - rgb0 * weight[:, None]) + rgb0 * mq_b[:, None]
    for name, rad in (("A", control_a), ("B", control_b)):
        zc = nref.z_scores(plain, rad.reshape(G, n, 3))
        print("control %s: z mean %.3f, max |z| %.3f" % (name, zc.mean(), np.abs(zc).max()))
        assert not nref.same_estimand(zc), name


# ---- 6. errors and zero work -------------------------------------------------------------------------------------------------------------------------
def test_errors_and_zero_work():
    L = _ffi.lib()
    ctx = core.Context(0)
    smoke = core.DeviceScene(ncs.media_flat(), ctx=ctx)
    many33 = core.DeviceScene(rcs.lamps32_flat(33), ctx=ctx)
    _, ds = _open("lamps-spheres")
    _, l8 = _open("lamps8")
    rays = np.ascontiguousarray(_inputs("lamps-spheres")[0][:8])
    mean, se, cnt = np.full((8, 3), -7.0), np.full(8, -7.0), np.full(4, 9, np.uint64)
    lamps = np.asarray(ds.lights(), np.int32)

    def call(scene, n_groups=8, group=1, g_first=0, depth=5, n_lights=0, prims=None, precision=0, r=rays, m=mean):
        return L.rtmi_render_rays_ris(scene.handle, precision, n_groups, group, g_first, core.ptr(r), None, 1, 0, depth, n_lights, core.ptr(prims), None,
                                      core.ptr(m), core.ptr(se), None, core.ptr(cnt))
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)
    # rtmi_render_rays' own errors come first, in their order, whatever the lights and the scene are
    assert call(smoke, n_groups=-1, n_lights=len(many), prims=many) == -1
    assert call(smoke, group=0) == -1 and call(smoke, g_first=-1) == -1 and call(smoke, depth=-1) == -1
    assert call(smoke, r=None, n_lights=len(many), prims=many) == -1 and call(smoke, m=None) == -1
    assert call(smoke, precision=7, n_lights=len(many), prims=many) == -1
    assert call(smoke, precision=1) == -3 and call(l8, precision=1) == -3        # RTMI_F32 on a mixed-kind scene
    # then the list's length, then zero work and the media, then the list's entries
    assert call(smoke, n_lights=len(many), prims=many) == -1 and b"n_lights" in L.rtmi_last_error()   # 33 lamps in a list
    assert call(smoke, n_lights=-1, prims=many) == -1
    assert call(smoke) == -3 and b"ConstantMedium" in L.rtmi_last_error()
    assert call(many33) == -1 and b"pass a list" in L.rtmi_last_error()                                  # 33 eligible lamps without a list
    assert call(ds, n_lights=1, prims=np.array([0], np.int32)) == -1 and call(ds, n_lights=1, prims=np.array([10 ** 6], np.int32)) == -1  # ineligible entries
    assert (mean == -7.0).all() and (se == -7.0).all() and (cnt == 9).all()         # a failed call writes nothing
    assert call(smoke, n_groups=0) == 0 and call(ds, n_groups=0, r=None, m=None) == 0 and (cnt == 9).all()
    assert call(ds, n_lights=len(lamps), prims=lamps) == 0 and cnt[1] == 8 and (mean != -7.0).all()
    assert call(many33, n_lights=32, prims=np.asarray(many33.lights(), np.int32)[:32]) == 0
    # the frame call refuses the same things behind its own checks, and n_tiles == 0 succeeds
    lin, err = np.full((8, 8, 3), -7.0), np.full((8, 8), -7.0)
    none = np.zeros(1, np.int32)

    def frame(scene, n_lights=0, prims=None, n_tiles=0, tiles=None, precision=0, s_count=1):
        return L.rtmi_render_lit_ris(scene.handle, precision, 8, 8, 0, s_count, 3, 1, n_lights, core.ptr(prims), n_tiles, core.ptr(tiles), None,
                                     core.ptr(lin), None, core.ptr(err), None, None, None)
    assert frame(smoke, s_count=0) == -1 and frame(smoke, n_tiles=2, tiles=np.array([0, 0], np.int32)) == -1
    assert frame(smoke) == -3 and frame(l8, precision=1) == -3 and frame(many33) == -1 and frame(ds, n_lights=len(many), prims=many) == -1
    assert frame(ds, n_lights=1, prims=np.array([0], np.int32), n_tiles=1, tiles=none) == -1
    assert (lin == -7.0).all() and (err == -7.0).all()
    assert frame(ds, n_tiles=0, tiles=none) == 0 and frame(smoke, n_tiles=0, tiles=none) == 0 and (lin == -7.0).all()
    assert frame(ds, n_tiles=1, tiles=none) == 0 and (lin != -7.0).all()
    # the probe refuses the same things, and the python layer raises
    for scene, code in ((smoke, -3), (many33, -1)):
        with pytest.raises(core.RtmiError) as ei:
            scene.probe_paths_ris(rays, np.arange(8, dtype=np.uint64))
        assert ei.value.code == code
        with pytest.raises(core.RtmiError) as ei:
            scene.render_rays_ris(rays)
        assert ei.value.code == code
    smoke.close(); many33.close(); ctx.close()


# ---- 7. the generators and the command line ----------------------------------------------------------------------------------------------------------
def test_render_with_and_the_command_line(tmp_path):
    _, sl = _open("lamps-spheres")
    view = dict(lookfrom=(6.0, 3.0, 9.0), lookat=(0.0, 1.0, 0.0), vup=(0.0, 1.0, 0.0))
    p = sl.render_with(camera.panorama_rays, 16, 8, 5, 5, depth=6, nee="ris", **view)
    q = sl.render_with(camera.panorama_rays, 16, 8, 5, 2, depth=6, nee="ris", **view)
    mis = sl.render_with(camera.panorama_rays, 16, 8, 5, 5, depth=6, nee="mis", **view)
    assert all(np.array_equal(x, y) for x, y in zip(p, q)) and p[3].tolist()[:2] == mis[3].tolist()[:2] and not np.array_equal(p[0], mis[0])
    name = str(tmp_path / "box.ppm")
    assert core.main([name, "13", "7", "3", "cornell-box-classic", "--lit", "ris", "--chunk", "2"]) == 0
    plain, lit = ((tmp_path / n).read_bytes() for n in ("box.ppm", "box.lit.ppm"))
    assert len(plain) == len(lit) and plain != lit and lit.startswith(b"P")
    name = str(tmp_path / "stop.ppm")  # with --adaptive: test_gpu_lit_tiles' --lit mis line, the estimator changed
    assert core.main([name, "21", "19", "12", "cornell-box-classic", "--lit", "ris", "--adaptive", "0.08", "--chunk", "4"]) == 0
    whole, stopped = (tmp_path / "stop.ppm").read_bytes(), (tmp_path / "stop.lit.ppm").read_bytes()
    assert len(whole) == len(stopped) and whole != stopped and stopped.startswith(b"P")
