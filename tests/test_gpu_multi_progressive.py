"""Progressive and adaptive frames on several devices (rtmi_render_adaptive_tiles_device, rtmi_assemble_progressive_device,
rtmi_render_multi_adaptive*), in one process with replicas that share device 0: the frame refined on n replicas is bit for bit the frame one
context refines.

Frame 37 x 21 (5 x 3 tiles, a partial right column and bottom row), the libm-free scenes of frame_reference.py, calls of 1, 3 and 4 samples (the
first leaves +inf standard errors in the records).  The numpy expectation comes from the oracle's individual samples
(multi_progressive_reference.py); linear, rgb8, stderr, samples and the ray counter are compared with np.array_equal -- the tolerance the
progressive, adaptive and frame tests hold these scenes to is zero -- and then with what one context returns from rtmi_render_progressive /
rtmi_render_adaptive after the same calls."""
import ctypes as C

import numpy as np
import pytest

import frame_reference as fr
import multi_progressive_reference as mp
import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import dist

pytestmark = pytest.mark.gpu

RTMI_E_ARG, RTMI_E_DEVICE, RTMI_E_STATE = -1, -2, -5
NX, NY = mp.SIZE
TILES = mp.n_tiles(NX, NY)
CASES = [("spheres", "f64"), ("mixed", "f64"), ("spheres", "f32")]
KW = dict(depth=fr.DEPTH, seed=fr.SEED)
_runs = {}


def _run(request, name, precision):
    if (name, precision) not in _runs:
        _runs[name, precision] = mp.Run(request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32"), name)
    return _runs[name, precision]


def _eq(got, exp, what):
    for a, b, label in zip(got, exp, ("linear", "rgb8", "stderr", "samples")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, label, a.dtype, b.dtype)
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            print("%s %s: %d elements differ, largest difference %g" % (what, label, int((a != b).sum()), float(np.nanmax(d))))
        assert np.array_equal(a, b), (what, label)


def _passes(ctx):
    v = C.c_int32()
    core.check(r._ffi.lib().rtmi_last_passes(ctx.handle, C.byref(v)))
    return v.value


class _Single:
    """one context with the scene: what the replicas are compared with"""

    def __init__(self, name, size=(NX, NY)):
        self.ctx = core.Context(0)
        self.ds = core.DeviceScene(fr.scene(name, *size), ctx=self.ctx)

    def close(self):
        self.ds.close()
        self.ctx.close()


@pytest.fixture
def closing():
    things = []
    yield things.append
    for t in reversed(things):
        t.close()


def _multi(closing, name, devices, size=(NX, NY), options=None):
    md = dist.MultiDevice(fr.scene(name, *size), devices, options=options)
    closing(md)
    return md


# ---- retire = 0: the progressive frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("name,precision", CASES, ids=["%s-%s" % c for c in CASES])
def test_progressive_equals_oracle_and_single_context(request, closing, name, precision, n):
    run = _run(request, name, precision)
    md, one = _multi(closing, name, [0] * n), _Single(name)
    closing(one)
    k = 0
    for s_count in mp.CHUNKS:
        lin, q, err, smp, cnt = md.render_multi_adaptive(NX, NY, k, s_count, 0, float("nan"), precision=precision, **KW)  # eps is not read
        slin, sq, serr, scnt = one.ds.render_progressive(NX, NY, k, s_count, precision=precision, **KW)
        k += s_count
        elin, eq, eerr, esmp, rays = run.expected(np.full((3, 5), k))
        assert np.isinf(err).all() if k == 1 else np.isfinite(err).all()
        _eq((lin, q, err, smp), (elin, eq, eerr, esmp), "n=%d k=%d vs the oracle's samples" % (n, k))
        assert (int(cnt[0]), int(cnt[1])) == (rays, NX * NY), (k, cnt)
        _eq((lin, q, err), (slin, sq, serr), "n=%d k=%d vs rtmi_render_progressive" % (n, k))
        assert np.array_equal(cnt, scnt) and (smp == k).all()
        assert md.progressive_samples() == k and md.adaptive_status() == (TILES, TILES, NX * NY * k)
        assert np.array_equal(md.adaptive_active_tiles(), np.arange(TILES))
    assert md.last_gather_path() == ("none" if n == 1 else "same-device")
    plin, pq, perr, pcnt = md.render_progressive(NX, NY, 0, 2, precision=precision, **KW)  # the driver: a new frame, DeviceScene's return shape
    assert plin.shape == (NY, NX, 3) and perr.shape == (NY, NX) and md.progressive_samples() == 2
    md.progressive_release()
    assert md.progressive_samples() == 0 and md.adaptive_status() == (0, 0, 0)


# ---- one-shot renders in between: the same gather, records and hand-off events on the same contexts --------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name,precision", CASES[:2], ids=["%s-%s" % c for c in CASES[:2]])
def test_one_shot_multi_renders_between_progressive_calls(closing, name, precision, n):
    """rtmi_render_multi and rtmi_render_multi_adaptive share plan_gather / enqueue_gather, c->multi and the ev_consumed hand-off: a one-shot render
    between two calls of a dealt progressive frame leaves the frame alone, and each is bit for bit what one context computes after the same calls."""
    md, one = _multi(closing, name, [0] * n), _Single(name)
    closing(one)

    def one_shot():
        lin, q, cnt = md.render(NX, NY, 4, precision=precision, **KW)
        slin, sq, scnt = one.ds.render(NX, NY, 4, precision=precision, **KW)
        for a, b, label in ((lin, slin, "linear"), (q, sq, "rgb8"), (cnt, scnt, "counters")):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), ("one-shot", n, label)
        assert md.last_gather_path() == "same-device"

    def progressive(s_first, s_count):
        lin, q, err, smp, cnt = md.render_multi_adaptive(NX, NY, s_first, s_count, 0, precision=precision, **KW)
        slin, sq, serr, scnt = one.ds.render_progressive(NX, NY, s_first, s_count, precision=precision, **KW)
        k = s_first + s_count
        _eq((lin, q, err), (slin, sq, serr), "n=%d k=%d vs rtmi_render_progressive" % (n, k))
        assert np.array_equal(cnt, scnt) and smp.dtype == np.int32 and (smp == k).all()
        assert md.progressive_samples() == one.ctx.progressive_samples() == k
        assert md.last_gather_path() == "same-device"

    one_shot()
    progressive(0, 2)
    one_shot()
    progressive(2, 3)  # a one-shot render does not touch the frame: the continuation is accepted and right


# ---- retire = 1: the adaptive frame ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name,precision", CASES, ids=["%s-%s" % c for c in CASES])
def test_adaptive_equals_schedule_and_single_context(request, closing, name, precision, n):
    run = _run(request, name, precision)
    eps, _ = run.choose_eps(call=1)
    rounds = run.schedule(eps)
    retired = TILES - int(rounds[1][2].sum())
    assert TILES / 4 <= retired <= 3 * TILES / 4, "after the second call %d of %d tiles have retired" % (retired, TILES)
    md, one = _multi(closing, name, [0] * n), _Single(name)
    closing(one)
    k = 0
    for s_count, (k_after, n_t, act) in zip(mp.CHUNKS, rounds):
        got = md.render_adaptive(NX, NY, k, s_count, eps, precision=precision, **KW)
        ref = one.ds.render_adaptive(NX, NY, k, s_count, eps, precision=precision, **KW)
        k += s_count
        assert k == k_after
        elin, eq, eerr, esmp, rays = run.expected(n_t)
        _eq(got[:4], (elin, eq, eerr, esmp), "n=%d k=%d vs the schedule" % (n, k))
        assert (int(got[4][0]), int(got[4][1])) == (rays, NX * NY), (k, got[4])
        merged = md.adaptive_active_tiles()
        assert merged.dtype == np.int32 and np.array_equal(merged, np.flatnonzero(act.ravel())), (k, "merged active list")
        _eq(got[:4], ref[:4], "n=%d k=%d vs rtmi_render_adaptive" % (n, k))
        assert np.array_equal(got[4], ref[4]) and np.array_equal(merged, one.ctx.adaptive_active_tiles())
        assert md.adaptive_status() == one.ctx.adaptive_status() == (int(act.sum()), TILES, int(esmp.sum()))
        for rk, ctx in enumerate(md.ctxs):  # every replica holds its own dealing of the list
            own = np.flatnonzero(act.ravel())
            assert np.array_equal(ctx.adaptive_active_tiles(), own[own % n == rk]), (k, rk)
    with pytest.raises(core.RtmiError) as e:  # the progressive rule cannot continue a frame in which a tile has retired
        md.render_multi_adaptive(NX, NY, k, 1, 0, precision=precision, **KW)
    assert e.value.code == RTMI_E_STATE and "retired" in str(e.value) and md.progressive_samples() == k


def test_refine_drivers_match_device_scene(request, closing):
    run = _run(request, "spheres", "f64")
    eps, _ = run.choose_eps(call=1)
    md, one = _multi(closing, "spheres", [0, 0]), _Single("spheres")
    closing(one)
    a = list(md.refine_adaptive(NX, NY, 8, 3, eps, first=1, **KW))
    b = list(one.ds.refine_adaptive(NX, NY, 8, 3, eps, first=1, **KW))
    assert len(a) == len(b) >= 3
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[6] == y[6] and all(np.array_equal(u, v) for u, v in zip(x[1:6], y[1:6]))
    a = list(md.refine(NX, NY, 5, 2, **KW))
    b = list(one.ds.refine(NX, NY, 5, 2, **KW))
    assert [x[0] for x in a] == [2, 4, 5] and all(np.array_equal(u, v) for x, y in zip(a, b) for u, v in zip(x[1:], y[1:]))
    a = list(md.refine_adaptive_denoised(NX, NY, 8, 4, 0.05, **KW))
    b = list(one.ds.refine_adaptive_denoised(NX, NY, 8, 4, 0.05, **KW))
    assert len(a) == len(b) >= 1
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[6] == y[6] and all(np.array_equal(u, v) for u, v in zip(x[1:6] + x[7:], y[1:6] + y[7:]))


# ---- the per-device primitive and the assemble -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES[:2], ids=["%s-%s" % c for c in CASES[:2]])
def test_dealt_primitive_records_and_assemble(request, closing, name, precision):
    import torch
    run = _run(request, name, precision)
    eps, _ = run.choose_eps(call=1)
    world, per = 3, mp.per_rank(NX, NY, 3)
    ranks = [_Single(name) for _ in range(world)]
    for s in ranks:
        closing(s)
    L = r._ffi.lib()
    assert [L.rtmi_local_tiles(NX, NY, rk, world) for rk in range(world)] == [len(mp.local_tiles(NX, NY, rk, world)) for rk in range(world)]
    poison = -7.0
    gathered = torch.full((world, per, 64, mp.REC), poison, dtype=torch.float64, device="cuda")
    counters = torch.zeros((world, 2), dtype=torch.int64, device="cuda")
    lin = torch.zeros((NY, NX, 3), dtype=torch.float64, device="cuda")
    q = torch.zeros((NY, NX, 3), dtype=torch.uint8, device="cuda")
    err = torch.zeros((NY, NX), dtype=torch.float64, device="cuda")
    smp = torch.zeros((NY, NX), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    k = 0
    for s_count, (_, n_t, act) in zip(mp.CHUNKS, run.schedule(eps)):
        for rk, s in enumerate(ranks):  # the records land where a gather would lay them
            s.ds.render_adaptive_tiles_device(NX, NY, k, s_count, 1, eps, rk, world, gathered[rk], counters[rk], precision=precision, **KW)
        k += s_count
        ranks[0].ctx.assemble_progressive_device(NX, NY, world, per, gathered, lin, q, err, smp)
        torch.cuda.synchronize()
        elin, eq, eerr, esmp, rays = run.expected(n_t)
        rec = gathered.cpu().numpy()
        exp = mp.gathered_records(elin, eerr, esmp, world)
        for rk in range(world):  # the primitive writes its local tiles only (out-of-image pixels: zeros); a padding slot is the caller's
            own = len(mp.local_tiles(NX, NY, rk, world))
            assert np.array_equal(rec[rk, :own], exp[rk, :own]), (k, rk, "records")
            assert (rec[rk, own:] == poison).all()
            assert ranks[rk].ctx.progressive_samples() == k
            mine = np.flatnonzero(act.ravel())
            assert np.array_equal(ranks[rk].ctx.adaptive_active_tiles(), mine[mine % world == rk]), (k, rk)
        cnt = counters.cpu().numpy()
        dealt_pixels = [int((exp[rk, :, :, 4] > 0).sum()) for rk in range(world)]  # a pixel inside the image holds at least one sample
        assert int(cnt[:, 0].sum()) == rays and [int(c) for c in cnt[:, 1]] == dealt_pixels and sum(dealt_pixels) == NX * NY
        _eq((lin.cpu().numpy(), q.cpu().numpy(), err.cpu().numpy(), smp.cpu().numpy()), mp.assemble(exp, NX, NY), "k=%d assembled" % k)
        _eq((lin.cpu().numpy(), q.cpu().numpy(), err.cpu().numpy(), smp.cpu().numpy()), (elin, eq, eerr, esmp), "k=%d frame" % k)
    # each output of the assemble may be NULL; too few slots is an argument error
    ranks[0].ctx.assemble_progressive_device(NX, NY, world, per, gathered, None, None, None, smp)
    torch.cuda.synchronize()
    assert L.rtmi_assemble_progressive_device(ranks[0].ctx.handle, NX, NY, world, per - 1, r._ffi.ptr(gathered), None, None, None, None, None) == RTMI_E_ARG


def test_tile_renderer_step_adaptive(request, closing):
    import torch
    run = _run(request, "spheres", "f64")
    eps, _ = run.choose_eps(call=1)
    one = _Single("spheres")
    closing(one)
    tr = dist.TileRenderer(one.ds, NX, NY, 0, 1)
    k = 0
    for s_count, (_, n_t, act) in zip(mp.CHUNKS, run.schedule(eps)):
        tr.step_adaptive(k, s_count, True, eps, **KW)
        k += s_count
        torch.cuda.synchronize()
        elin, eq, eerr, esmp, rays = run.expected(n_t)
        _eq((tr.linear.cpu().numpy(), tr.rgb8.cpu().numpy(), tr.stderr.cpu().numpy(), tr.samples.cpu().numpy()), (elin, eq, eerr, esmp), "k=%d" % k)
        assert [int(v) for v in tr.counters.cpu()] == [rays, NX * NY] and one.ctx.adaptive_status()[0] == int(act.sum())


# ---- the same bytes however a call is split into sample passes ------------------------------------------------------------------------------
def test_workspace_bytes_split_leaves_the_images_unchanged(closing):
    nx, ny = fr.SIZE_PASSES["spheres"]  # 338 tiles, 169 per replica: at the option's floor of 1 MiB a pass holds 4 samples of them
    chunks = (5, 5, 5)
    one = _Single("spheres", (nx, ny))
    closing(one)
    _, _, err, _ = one.ds.render_progressive(nx, ny, 0, 10, **KW)
    tx, ty = fr.tiles_of(nx, ny)
    pad = np.full((ty * 8, tx * 8), -np.inf)
    pad[:ny, :nx] = err
    worst = np.sort(pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).ravel())
    eps = float(0.5 * (worst[len(worst) // 2 - 1] + worst[len(worst) // 2]))

    def run(md, retire):
        out, passes, k = [], [], 0
        for s_count in chunks:
            out.append(md.render_multi_adaptive(nx, ny, k, s_count, retire, eps, **KW))
            passes.append([_passes(ctx) for ctx in md.ctxs])
            k += s_count
        return out, passes, md.adaptive_active_tiles()

    md0 = _multi(closing, "spheres", [0, 0], (nx, ny))
    md = _multi(closing, "spheres", [0, 0], (nx, ny), options={"workspace_bytes": 1 << 20})
    flat0, p0, _ = run(md0, 0)
    flat, p1, _ = run(md, 0)  # the progressive rule: every call of every replica is split
    assert all(p == 1 for call in p0 for p in call) and all(p > 1 for call in p1 for p in call), (p0, p1)
    for a, b in zip(flat0, flat):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    whole, _, active = run(md0, 1)
    assert 0 < len(active) < tx * ty, "the frame must hold retired and active tiles"
    split, p1, active2 = run(md, 1)  # the adaptive rule: a call is split while enough tiles are active (the first is)
    assert all(p > 1 for p in p1[0]), p1
    assert np.array_equal(active, active2)
    for a, b in zip(whole, split):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    k = 0
    for s_count, a in zip(chunks, whole):  # ... and they are the single context's
        ref = one.ds.render_adaptive(nx, ny, k, s_count, eps, **KW)
        k += s_count
        assert all(np.array_equal(u, v) for u, v in zip(a, ref))
    assert np.array_equal(active, one.ctx.adaptive_active_tiles())


# ---- the one-rank communicator path ------------------------------------------------------------------------------------------------------------
def test_rccl_gather_with_one_replica_equals_the_copy_path(request, closing, monkeypatch):
    run = _run(request, "spheres", "f64")
    eps, _ = run.choose_eps(call=1)

    def frames(md):
        out, k = [], 0
        for s_count in mp.CHUNKS:
            out.append(md.render_adaptive(NX, NY, k, s_count, eps, **KW))
            k += s_count
        return out

    plain = _multi(closing, "spheres", [0])
    a = frames(plain)
    assert plain.last_gather_path() == "none"
    monkeypatch.setenv("RTMI_MULTI_GATHER", "rccl")
    forced = _multi(closing, "spheres", [0])
    b = frames(forced)
    assert forced.last_gather_path() == "rccl"
    two = _multi(closing, "spheres", [0, 0])
    with pytest.raises(core.RtmiError) as e:  # RCCL refuses one device twice: an argument error, reported before anything is launched
        two.render_adaptive(NX, NY, 0, 2, eps, **KW)
    assert e.value.code == RTMI_E_ARG and "distinct devices" in str(e.value) and two.progressive_samples() == 0
    monkeypatch.delenv("RTMI_MULTI_GATHER")
    for x, y, (_, n_t, _) in zip(a, b, run.schedule(eps)):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
        _eq(y[:4], run.expected(n_t)[:4], "rccl, one replica")


# ---- retirement by a caller's map ------------------------------------------------------------------------------------------------------------
def test_retire_by_map_on_multi_device(closing):
    md, one = _multi(closing, "spheres", [0, 0, 0]), _Single("spheres")
    closing(one)
    md.render_adaptive(NX, NY, 0, 4, 0.0, **KW)
    before = md.adaptive_active_tiles()
    chosen = np.array([1, 4, 7, 13], np.int32)  # one tile of every replica and two of replica 1; 4 and 13 lie on the partial column / row
    assert set(chosen) <= set(before)
    noise = np.ones((NY, NX))
    tx = fr.tiles_of(NX, NY)[0]
    for g in chosen:
        noise[(g // tx) * 8:(g // tx) * 8 + 8, (g % tx) * 8:(g % tx) * 8 + 8] = 0.25
    noise[0, 0] = np.nan  # tile 0 is not chosen: a NaN fails
    assert md.adaptive_retire(noise, 0.5) == len(chosen)
    after = md.adaptive_active_tiles()
    assert np.array_equal(after, np.setdiff1d(before, chosen))
    lin, q, err, smp, cnt = md.render_adaptive(NX, NY, 4, 4, 0.0, **KW)
    assert np.array_equal(md.adaptive_active_tiles(), after)
    n_t = np.where(np.isin(np.arange(TILES).reshape(3, 5), after), 8, 4)  # the chosen tiles (and any the first call retired) stopped at 4
    assert np.array_equal(smp, np.repeat(np.repeat(n_t, 8, 0), 8, 1)[:NY, :NX]) and set(np.unique(smp)) == {4, 8}
    for level in np.unique(smp):  # every pixel is the one-shot render with as many samples as its tile holds
        rlin, rq, _ = one.ds.render(NX, NY, int(level), **KW)
        sel = smp == level
        assert np.array_equal(lin[sel], rlin[sel]) and np.array_equal(q[sel], rq[sel]), level
    assert md.adaptive_status() == (len(after), TILES, int(smp.sum()))


# ---- failures ------------------------------------------------------------------------------------------------------------------------------------
def test_failure_on_one_replica_drops_every_frame(request, closing):
    run = _run(request, "spheres", "f64")
    md = _multi(closing, "spheres", [0, 0, 0])
    md.render_multi_adaptive(NX, NY, 0, 1, 1, 0.0, **KW)
    md.ctxs[1].set_option("test_fail_next_render", 1)
    with pytest.raises(core.RtmiError) as e:
        md.render_multi_adaptive(NX, NY, 1, 3, 1, 0.0, **KW)
    assert e.value.code == RTMI_E_DEVICE and "test_fail_next_render" in str(e.value)
    assert [ctx.progressive_samples() for ctx in md.ctxs] == [0, 0, 0]
    for s_first in (1, 4):  # neither the old k nor the k replica 0 had reached continues anything
        with pytest.raises(core.RtmiError) as e:
            md.render_multi_adaptive(NX, NY, s_first, 3, 1, 0.0, **KW)
        assert e.value.code == RTMI_E_STATE
    for rk, ctx in enumerate(md.ctxs):  # ... on any replica
        rc = r._ffi.lib().rtmi_render_adaptive_tiles_device(md.scenes[rk].handle, NX, NY, 1, 3, 1, 0.0, fr.DEPTH, fr.SEED, 0, rk, 3, None, None, None)
        assert rc == RTMI_E_STATE
    k = 0
    for s_count in mp.CHUNKS:  # s_first = 0 works again
        got = md.render_multi_adaptive(NX, NY, k, s_count, 0, **KW)
        k += s_count
        _eq(got[:4], run.expected(np.full((3, 5), k))[:4], "after the failure, k=%d" % k)
    # the hook on replica 0, in a continuation: nothing was launched anywhere, every frame stays
    md.ctxs[0].set_option("test_fail_next_render", 1)
    with pytest.raises(core.RtmiError):
        md.render_multi_adaptive(NX, NY, k, 2, 0, **KW)
    assert [ctx.progressive_samples() for ctx in md.ctxs] == [k, k, k]


def test_dealing_mismatch_is_refused_and_leaves_the_frames(request, closing):
    run = _run(request, "spheres", "f64")
    md = _multi(closing, "spheres", [0, 0, 0])
    L = r._ffi.lib()
    md.render_multi_adaptive(NX, NY, 0, 1, 0, **KW)
    two = (C.c_void_p * 2)(md.scenes[0].handle, md.scenes[1].handle)
    rc = L.rtmi_render_multi_adaptive(2, two, NX, NY, 1, 3, 0, 0.0, fr.DEPTH, fr.SEED, 0, None, None, None, None, None)
    assert rc == RTMI_E_STATE and "dealing" in L.rtmi_last_error().decode() and "stride 3" in L.rtmi_last_error().decode()
    rc = L.rtmi_render_adaptive_tiles_device(md.scenes[2].handle, NX, NY, 1, 3, 0, 0.0, fr.DEPTH, fr.SEED, 0, 1, 3, None, None, None)
    assert rc == RTMI_E_STATE and "dealing" in L.rtmi_last_error().decode()
    # the whole-frame entries are the dealing (0, 1): they do not continue a frame dealt (0, 3)
    rc = L.rtmi_render_progressive(md.scenes[0].handle, NX, NY, 1, 3, fr.DEPTH, fr.SEED, 0, 0, 0, NX, NY, None, None, None, None)
    assert rc == RTMI_E_STATE and "dealing" in L.rtmi_last_error().decode()
    assert [ctx.progressive_samples() for ctx in md.ctxs] == [1, 1, 1]
    got = md.render_multi_adaptive(NX, NY, 1, 3, 0, **KW)
    _eq(got[:4], run.expected(np.full((3, 5), 4))[:4], "the correct continuation")


def test_whole_frame_entries_continue_a_dealt_0_1_frame(request, closing):
    import torch
    run = _run(request, "spheres", "f64")
    one = _Single("spheres")
    closing(one)
    rec = torch.zeros((TILES, 64, mp.REC), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    one.ds.render_adaptive_tiles_device(NX, NY, 0, 1, 0, 0.0, 0, 1, rec, None, **KW)
    lin, q, err, cnt = one.ds.render_progressive(NX, NY, 1, 3, **KW)  # rtmi_render_progressive continues what the tiles call started
    elin, eq, eerr, esmp, rays = run.expected(np.full((3, 5), 4))
    _eq((lin, q, err), (elin, eq, eerr), "progressive after tiles")
    assert (int(cnt[0]), int(cnt[1])) == (rays, NX * NY)
    one.ds.render_adaptive_tiles_device(NX, NY, 4, 4, 0, 0.0, 0, 1, rec, None, **KW)  # ... and the other way round
    elin, eq, eerr, esmp, rays = run.expected(np.full((3, 5), 8))
    assert np.array_equal(rec.cpu().numpy(), mp.dealt_records(elin, eerr, esmp, 0, 1))


# ---- distinct devices --------------------------------------------------------------------------------------------------------------------------
def test_two_distinct_devices(request, closing):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: the gather between devices needs two (the shared-device form is tested above)")
    run = _run(request, "spheres", "f64")
    eps, _ = run.choose_eps(call=1)
    md = _multi(closing, "spheres", [0, 1])
    k = 0
    for s_count, (_, n_t, act) in zip(mp.CHUNKS, run.schedule(eps)):
        got = md.render_adaptive(NX, NY, k, s_count, eps, **KW)
        k += s_count
        _eq(got[:4], run.expected(n_t)[:4], "two devices, k=%d" % k)
        assert np.array_equal(md.adaptive_active_tiles(), np.flatnonzero(act.ravel()))
    assert md.last_gather_path() in ("rccl", "peer-copy")
