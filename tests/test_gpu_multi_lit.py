"""Light-sampled frames on several devices (rtmi_lit_tiles_records_device, rtmi_multi_lit_*), in one process with replicas that share device 0: the
frame refined on n replicas is bit for bit the frame one context refines.

Every comparison is np.array_equal on the arrays one context's calls return -- rtmi_render_lit_device / rtmi_render_lit_vol_device /
rtmi_render_lit_ris_device through one state over the same chunks, DeviceScene.refine_lit_adaptive for the adaptive runs -- which test_gpu_lit*.py,
test_gpu_vol.py and test_gpu_ris.py pin.  The record, the dealing, the padding, the assembly and the retire rule are multi_lit_reference's
(test_multi_lit_host.py).  Frame 37 x 21 (5 x 3 tiles, a partial right column and bottom row), depth 6, calls of 1, 3 and 4 samples (the first leaves
+inf standard errors in the records)."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import frame_reference as fr
import lit_cases as lc
import multi_lit_reference as ml
from raytrace_clj_amd import _ffi, core, dist
from tests import direct_cases as dcs
from tests import ris_cases as rcs
from tests import vol_cases as vcs

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED, E_STATE = -1, -3, -5
NX, NY = ml.SIZE
TILES = ml.n_tiles(NX, NY)
DEPTH = 6
SEED = lc.SEED
POISON = -7.0
FLAT = {"dc": dc.flat, "dcs": dcs.flat, "vcs": vcs.flat, "rcs": rcs.flat}
# (family, scene, estimator, light_choice, volume, precision)
CONFIGS = ([("dcs", name, est, choice, False, "f64") for name in ("sphere-lamp", "cornell")
            for est, choice in (("plain", 0), ("nee", 0), ("mis", 0), ("mis", 1))] +
           [("rcs", "lamps8", "ris", 0, False, "f64"), ("vcs", "smoke", "nee", 0, True, "f64"), ("vcs", "smoke", "mis", 0, True, "f64"),
            ("dcs", "sphere-lamp", "mis", 0, False, "f32")])
IDS = ["%s-%s%s%s-%s" % (c[1], c[2], ":power" if c[3] else "", "-vol" if c[4] else "", c[5]) for c in CONFIGS]
MIS = CONFIGS[2]


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    """(family, name) -> DeviceScene on the module's context, made once"""
    made = {}

    def get(family, name):
        if (family, name) not in made:
            made[family, name] = core.DeviceScene(FLAT[family](name), ctx=ctx)
        return made[family, name]

    yield get
    for ds in made.values():
        ds.close()


@pytest.fixture
def closing():
    things = []
    yield things.append
    for t in reversed(things):
        t.close()


def _multi(closing, config, n, devices=None, options=None):
    md = dist.MultiDevice(FLAT[config[0]](config[1]), [0] * n if devices is None else devices, options=options)
    closing(md)
    return md


def _kw(config):
    return dict(estimator=config[2], light_choice=config[3], volume=config[4], precision=config[5], depth=DEPTH, seed=SEED)


def _single_call(ds, config, nx, ny, s_first, s_count, b, seed=SEED):
    """one context's frame call into the HBM buffers b (state, lin, se, q, cnt)"""
    _, _, est, choice, volume, precision = config
    kw = dict(depth=DEPTH, seed=seed, precision=precision, state=b["state"], out_counters=b["cnt"])
    if est == "ris":
        ds.render_lit_ris_device(nx, ny, s_first, s_count, b["lin"], b["se"], b["q"], **kw)
    elif volume:
        ds.render_lit_vol_device(nx, ny, s_first, s_count, b["lin"], b["se"], b["q"], estimator=est, light_choice=choice, **kw)
    else:
        ds.render_lit_device(nx, ny, s_first, s_count, b["lin"], b["se"], b["q"], estimator=est, light_choice=choice, **kw)


def _buffers(nx, ny):
    import torch
    f64 = dict(dtype=torch.float64, device=_dev())
    b = dict(state=torch.zeros((nx * ny, _ffi.RAYS_REC), **f64), lin=torch.zeros((ny, nx, 3), **f64), se=torch.zeros((ny, nx), **f64),
             q=torch.zeros((ny, nx, 3), dtype=torch.uint8, device=_dev()), cnt=torch.zeros(4, dtype=torch.int64, device=_dev()))
    torch.cuda.synchronize(_dev())
    return b


_singles = {}


def _single(scenes, config, size=(NX, NY), chunks=ml.CHUNKS, seed=SEED):
    """what one context holds after every call of `chunks` through one state: [(linear, rgb8, stderr, samples int32, counters uint64)], computed once
    per configuration and shared; do not write into it"""
    import torch
    key = (config, size, tuple(chunks), seed)
    if key not in _singles:
        nx, ny = size
        ds, b, out, k = scenes(config[0], config[1]), _buffers(nx, ny), [], 0
        for n in chunks:
            _single_call(ds, config, nx, ny, k, n, b, seed)
            k += n
            torch.cuda.synchronize(_dev())
            out.append((b["lin"].cpu().numpy(), b["q"].cpu().numpy(), b["se"].cpu().numpy(),
                        b["state"][:, 9].reshape(ny, nx).cpu().numpy().astype(np.int32), b["cnt"].cpu().numpy().astype(np.uint64)))
        _singles[key] = out
    return _singles[key]


def _eq(got, exp, what):
    for a, b, label in zip(got, exp, ("linear", "rgb8", "stderr", "samples", "counters")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, label, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            print("%s %s: %d elements differ, largest difference %g" % (what, label, int((a != b).sum()), float(np.nanmax(d))))
        assert np.array_equal(a, b), (what, label)


# ---- uniform frames ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ml.WORLDS)
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_uniform_frames_equal_the_single_context(scenes, closing, config, n):
    """n = 8 pads a slot on the last ranks (15 tiles, two slots each); every call's linear, rgb8, stderr, samples and four counters are one context's"""
    want = _single(scenes, config)
    md = _multi(closing, config, n)
    k, total = 0, np.zeros(4, np.uint64)
    for s_count, exp in zip(ml.CHUNKS, want):
        got = md.lit_render(NX, NY, s_count, **_kw(config))
        k += s_count
        assert np.isinf(got[2]).all() if k == 1 else np.isfinite(got[2]).all()
        _eq(got, exp, "%s n=%d k=%d" % (config[1:], n, k))
        total += got[4]
        assert md.lit_status(NX, NY) == (k, TILES) and (got[3] == k).all() and int(got[4][1]) == NX * NY * s_count
        assert (int(got[4][2]) > 0) == (config[2] != "plain"), got[4]
    assert np.array_equal(md.lit_active_tiles(NX, NY), np.arange(TILES, dtype=np.int32))
    assert md.last_gather_path() == ("none" if n == 1 else "same-device")
    # the drivers: a fresh frame each, DeviceScene's return shapes, the counters summed over the calls
    lin, q, err, cnt = md.render_lit(NX, NY, sum(ml.CHUNKS), chunk=3, **_kw(config))
    _eq((lin, q, err), want[-1][:3], "render_lit")
    assert np.array_equal(cnt, total) and np.array_equal(total, sum(w[4] for w in want))
    ks = [out[0] for out in md.refine_lit(NX, NY, 5, 4, **_kw(config))]
    assert ks == [4, 5] and md.lit_status(NX, NY) == (5, TILES)


def test_a_replica_with_no_tile(scenes, closing):
    """9 x 9 is four tiles: of eight replicas four own none, launch no trace, and hand zeros to the gather"""
    nx, ny = ml.SMALL
    want = _single(scenes, MIS, ml.SMALL, (1, 3))
    md = _multi(closing, MIS, 8)
    for s_count, exp in zip((1, 3), want):
        _eq(md.lit_render(nx, ny, s_count, **_kw(MIS)), exp, "9 x 9 on 8 replicas")
    assert md.lit_status(nx, ny) == (4, 4) and md.lit_active_tiles(nx, ny).tolist() == [0, 1, 2, 3]
    assert md.lit_retire(nx, ny, 1e30) == 0 and md.lit_status(nx, ny) == (4, 0)  # every tile retires; a render of nothing is legal and changes nothing
    again = md.lit_render(nx, ny, 2, **_kw(MIS))
    _eq(again[:4], want[-1][:4], "a call with no tile listed")
    assert not again[4].any() and md.lit_status(nx, ny) == (6, 0)


# ---- the primitive -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [MIS, CONFIGS[-1]], ids=["f64", "f32"])
def test_records_primitive(ctx, scenes, config):
    """rtmi_lit_tiles_records_device on poisoned buffers: the records are the numpy restatement's, padded slots and outside pixels are zeros, nothing
    past n_slots is written, and laid out as a gather lays them they assemble through rtmi_assemble_progressive_device to the single context's planes,
    the 8-bit frame included: the assemble's quantiser and rtmi_render_lit's give the same bytes"""
    import torch
    ds, b = scenes(config[0], config[1]), _buffers(NX, NY)
    _single_call(ds, config, NX, NY, 0, 1, b)
    every = torch.arange(TILES, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize(_dev())
    some = every[::2].contiguous()  # a second call on every other tile: the samples differ from tile to tile, and one-sample tiles keep +inf
    ds.render_lit_tiles_device(NX, NY, 1, 3, len(some), some, b["lin"], b["se"], b["q"], estimator=config[2], state=b["state"], depth=DEPTH, seed=SEED,
                               precision=config[5])
    torch.cuda.synchronize(_dev())
    state, lin, se, q = (b[k].cpu().numpy() for k in ("state", "lin", "se", "q"))
    smp = state[:, 9].reshape(NY, NX).astype(np.int32)
    assert set(np.unique(smp)) == {1, 4} and np.isinf(se).any() and np.isfinite(se).any()
    guard = 2
    for first, stride, slots in ((0, 1, TILES), (0, 1, TILES + 3), (1, 2, 7), (2, 3, 5), (7, 8, 2), (14, 8, 2), (15, 1, 1), (3, 4, 0)):
        rec = torch.full((slots + guard, 64, ml.REC), POISON, dtype=torch.float64, device=_dev())
        torch.cuda.synchronize(_dev())
        ctx.lit_tiles_records_device(NX, NY, first, stride, slots, b["state"], b["lin"], b["se"], rec)
        torch.cuda.synchronize(_dev())
        got = rec.cpu().numpy()
        exp = ml.records(state, lin, se, NX, NY, first, stride, slots)
        assert np.array_equal(got[:slots].view(np.uint64), exp.view(np.uint64)), (first, stride, slots)
        assert (got[slots:] == POISON).all(), (first, stride, slots, "guard rows")
    for n in (1, 3, 8):
        per = ml.per_replica(NX, NY, n)
        g = torch.full((n, per, 64, ml.REC), POISON, dtype=torch.float64, device=_dev())
        out = _buffers(NX, NY)
        out_smp = torch.full((NY, NX), -1, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize(_dev())
        for r in range(n):
            ctx.lit_tiles_records_device(NX, NY, r, n, per, b["state"], b["lin"], b["se"], g[r])
        ctx.assemble_progressive_device(NX, NY, n, per, g, out["lin"], out["q"], out["se"], out_smp)
        torch.cuda.synchronize(_dev())
        assert np.array_equal(g.cpu().numpy().view(np.uint64), ml.gathered(state, lin, se, NX, NY, n).view(np.uint64)), n
        _eq((out["lin"].cpu().numpy(), out["q"].cpu().numpy(), out["se"].cpu().numpy(), out_smp.cpu().numpy()), (lin, q, se, smp), "assembled, n=%d" % n)
        assert np.array_equal(q, ml.quantise(lin))


# ---- adaptive ------------------------------------------------------------------------------------------------------------------------------------
ADAPTIVE = {"mis": (MIS, {}), "denoised": (CONFIGS[6], dict(denoised=True)), "ris": (CONFIGS[8], {})}
_adaptive = {}


def _adaptive_single(scenes, which):
    """The single context's adaptive run (first 2, chunk 3, cap 11) at an eps chosen HERE, by running it: the thresholds tried are quantiles of the
    per-tile maxima of the single context's own noise map after the second round's samples, and the first under which the run retires some but not
    all tiles by the end of its second round is kept -> (eps, DeviceScene.refine_lit_adaptive's tuple)"""
    if which not in _adaptive:
        config, more = ADAPTIVE[which]
        ds = scenes(config[0], config[1])
        kw = dict(estimator=config[2], light_choice=config[3], depth=DEPTH, seed=SEED)
        probe = ds.refine_lit_adaptive(NX, NY, 5, 3, 0.0, first=2, **kw)  # eps 0: nothing but exact tiles retires; the planes after k = 5
        noise = probe[2]
        if more:
            noise = ds.ctx.denoise(probe[0], probe[2], ds.render_features(NX, NY, core.FEATURE_SAMPLES, SEED)[0])[2]
        tx, ty = ml.tiles_xy(NX, NY)
        peaks = np.sort([np.max(noise[y * 8:y * 8 + 8, x * 8:x * 8 + 8]) for y in range(ty) for x in range(tx)])
        peaks = peaks[np.isfinite(peaks)]
        for q in (0.5, 0.35, 0.65, 0.2, 0.8):
            i = int(q * (len(peaks) - 1))
            eps = float(0.5 * (peaks[i] + peaks[i + 1]))
            run = ds.refine_lit_adaptive(NX, NY, 11, 3, eps, first=2, **kw, **more)
            if len(run[5]) >= 2 and 0 < len(run[5][1][1]) < TILES:
                _adaptive[which] = (eps, run)
                break
        assert which in _adaptive, "no threshold retires some but not all tiles by the second round"
    return _adaptive[which]


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("which", sorted(ADAPTIVE))
def test_adaptive_equals_the_single_context(scenes, closing, which, n):
    config, more = ADAPTIVE[which]
    eps, (slin, sq, serr, ssmp, scnt, srounds) = _adaptive_single(scenes, which)
    md = _multi(closing, config, n)
    lin, q, err, smp, cnt, rounds = md.refine_lit_adaptive(NX, NY, 11, 3, eps, first=2, estimator=config[2], light_choice=config[3], depth=DEPTH, seed=SEED, **more)
    assert [k for k, _ in rounds] == [k for k, _ in srounds], (rounds, srounds)
    for (k, got), (_, exp) in zip(rounds, srounds):
        assert got.dtype == np.int32 and np.array_equal(got, exp), (which, n, k, got, exp)
    _eq((lin, q, err, smp, cnt), (slin, sq, serr, ssmp, scnt), "adaptive %s n=%d" % (which, n))
    assert len(np.unique(smp)) > 1 and md.lit_status(NX, NY) == (rounds[-1][0], len(rounds[-1][1]))


# ---- retire by a caller's map --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("on_device", [False, True], ids=["host-map", "device-map"])
def test_retire_by_a_callers_map(scenes, closing, n, on_device):
    import torch
    want = _single(scenes, MIS, chunks=(2, 3))
    md = _multi(closing, MIS, n)
    _eq(md.lit_render(NX, NY, 2, **_kw(MIS)), want[0], "before the map")
    noise = np.full((NY, NX), 0.5)
    noise[0:8, 8:16] = 0.01       # tile 1 passes
    noise[16:21, 32:37] = 0.01    # tile 14, partial on both edges, passes on the pixels it has
    noise[8:16, 0:8] = 0.01
    noise[9, 3] = np.nan          # tile 5: a NaN fails
    lists = [ml.survivors(noise, 0.1, ml.owned(NX, NY, r, n), NX, NY) for r in range(n)]  # the rule on each replica's own list
    keep = ml.merged(lists)
    assert keep.tolist() == [t for t in range(TILES) if t not in (1, 14)]
    given = torch.from_numpy(noise).to(_dev()) if on_device else noise
    torch.cuda.synchronize(_dev())
    assert md.lit_retire(NX, NY, 0.1, given) == len(keep) and np.array_equal(md.lit_active_tiles(NX, NY), keep)
    assert md.lit_status(NX, NY) == (2, len(keep))
    lin, q, err, smp, cnt = md.lit_render(NX, NY, 3, **_kw(MIS))
    took = np.zeros(TILES, bool)
    took[keep] = True
    mask = np.repeat(np.repeat(took.reshape(3, 5), 8, axis=0), 8, axis=1)[:NY, :NX]
    assert np.array_equal(smp, np.where(mask, 5, 2).astype(np.int32)) and int(cnt[1]) == 3 * int(mask.sum())
    for got, a, b in ((lin, want[1][0], want[0][0]), (q, want[1][1], want[0][1]), (err, want[1][2], want[0][2])):
        m = mask if got.ndim == 2 else mask[..., None]
        assert np.array_equal(got, np.where(m, a, b))  # a retired tile keeps every bit; a listed one is the uninterrupted frame's


def test_retire_by_a_map_still_being_written_on_replica_0s_stream(scenes, closing):
    """The device form's contract: the map is complete on replica 0's CONTEXT STREAM, not on the host's clock.  203 x 99 (338 tiles) on three replicas:
    the denoiser is enqueued on replica 0's stream into a buffer poisoned with NaN (a NaN fails the rule: a replica that read the buffer early would
    keep every tile) and the retirement follows at once, without a synchronisation in between; every replica's copy of the map is ordered behind
    the filter, so the lists are the numpy rule's on the filtered map."""
    import torch
    nx, ny = fr.SIZE_PASSES["spheres"]
    tiles = ml.n_tiles(nx, ny)
    md = _multi(closing, MIS, 3)
    f64 = dict(dtype=torch.float64, device=_dev())
    lin, err, ferr = torch.zeros((ny, nx, 3), **f64), torch.zeros((ny, nx), **f64), torch.full((ny, nx), float("nan"), **f64)
    torch.cuda.synchronize(_dev())
    md.lit_render_device(nx, ny, 4, lin, None, err, None, None, **_kw(MIS))
    want = md.ctxs[0].denoise(lin.cpu().numpy(), err.cpu().numpy())[2]  # the same filter through the host form: the map the device form will hold
    tx, ty = ml.tiles_xy(nx, ny)
    peaks = np.sort([np.max(want[y * 8:y * 8 + 8, x * 8:x * 8 + 8]) for y in range(ty) for x in range(tx)])
    eps = float(0.5 * (peaks[tiles // 2 - 1] + peaks[tiles // 2]))
    keep = ml.merged([ml.survivors(want, eps, ml.owned(nx, ny, r, 3), nx, ny) for r in range(3)])
    assert 0 < len(keep) < tiles
    md.ctxs[0].denoise_device(nx, ny, lin, err, None, None, None, ferr)  # asynchronous, on replica 0's context stream
    left = md.lit_retire(nx, ny, eps, ferr)
    torch.cuda.synchronize(_dev())
    assert np.array_equal(ferr.cpu().numpy(), want, equal_nan=True)
    assert left == len(keep) and np.array_equal(md.lit_active_tiles(nx, ny), keep)


# ---- key and failure rules -----------------------------------------------------------------------------------------------------------------------
def _refused(md, code, *words, **kw):
    before = md.lit_status(NX, NY), md.lit_active_tiles(NX, NY).tolist()
    with pytest.raises(core.RtmiError) as e:
        md.lit_render(NX, NY, 3, **kw)
    assert e.value.code == code and all(w in str(e.value) for w in words), (e.value.code, str(e.value))
    assert (md.lit_status(NX, NY), md.lit_active_tiles(NX, NY).tolist()) == before


def test_refusals_launch_and_change_nothing(scenes, closing):
    """each refusal is followed by a valid call, and the frame then equals the uninterrupted run's"""
    want = _single(scenes, MIS)
    md = _multi(closing, MIS, 2)
    kw = _kw(MIS)
    lamps = scenes("dcs", "sphere-lamp").lights().tolist()
    no_lamp = [p for p in range(7) if p not in lamps][:1]
    assert len(lamps) == 1 and no_lamp
    _refused(md, E_ARG, "replica 0", **dict(kw, lights=no_lamp))  # a ball is no lamp: the sibling's light check, before the first launch
    _eq(md.lit_render(NX, NY, 1, **kw), want[0], "after a refused light list")
    _refused(md, E_STATE, "seed %d" % SEED, "seed %d" % (SEED + 1), **dict(kw, seed=SEED + 1))  # both keys are in the text
    _refused(md, E_STATE, "depth 6", "depth 7", **dict(kw, depth=7))
    _refused(md, E_STATE, "estimator 2", "estimator 1", **dict(kw, estimator="nee"))
    _refused(md, E_STATE, "lights NULL", "lights [%d]" % lamps[0], **dict(kw, lights=lamps))  # the same lamp, but listed: another key
    _eq(md.lit_render(NX, NY, 3, **kw), want[1], "after refused keys")
    # an edit changes the scenes' revisions: the frame is not continued across it ...
    f = dcs.flat("sphere-lamp")
    cam = np.array(f.cam, np.float64)
    assert int(f.cam_kind) == 1 and cam[21] == 0.0
    cam[21] = 0.3
    md.set_camera((1, cam))
    _refused(md, E_STATE, "revisions", **kw)
    # ... it is reset, and is then the fresh frame of the edited scene
    md.lit_reset(NX, NY)
    assert md.lit_status(NX, NY) == (0, TILES)
    one = core.DeviceScene(f, ctx=scenes("dcs", "sphere-lamp").ctx)
    closing(one)
    one.set_camera((1, cam))
    b, k = _buffers(NX, NY), 0
    for s_count in ml.CHUNKS:
        import torch
        _single_call(one, MIS, NX, NY, k, s_count, b)
        k += s_count
        torch.cuda.synchronize(_dev())
        exp = (b["lin"].cpu().numpy(), b["q"].cpu().numpy(), b["se"].cpu().numpy(), b["state"][:, 9].reshape(NY, NX).cpu().numpy().astype(np.int32),
               b["cnt"].cpu().numpy().astype(np.uint64))
        _eq(md.lit_render(NX, NY, s_count, **kw), exp, "the edited scene, k=%d" % k)
    assert not np.array_equal(exp[0], want[-1][0])  # (the lens moved the rays)


def test_media_mode_is_refused_before_anything_is_launched(scenes, closing):
    smoke = CONFIGS[9]
    want = _single(scenes, smoke)
    md = _multi(closing, smoke, 3)
    _refused(md, E_UNSUPPORTED, "ConstantMedium", **dict(_kw(smoke), volume=False))  # estimator 1, volume 0 on a scene that holds media
    with pytest.raises(ValueError):
        md.lit_render(NX, NY, 1, **dict(_kw(smoke), estimator="ris", volume=True))
    k = 0
    for s_count, exp in zip(ml.CHUNKS, want):
        _eq(md.lit_render(NX, NY, s_count, **_kw(smoke)), exp, "smoke after the refusal")
    _refused(md, E_STATE, "volume 1", "volume 0", **dict(_kw(smoke), volume=False))  # mid-frame the key speaks first


def test_reset_then_render_equals_a_fresh_frame(scenes, closing):
    want = _single(scenes, MIS)
    md = _multi(closing, MIS, 3)
    md.lit_render(NX, NY, 2, **dict(_kw(MIS), seed=SEED + 5))
    assert md.lit_retire(NX, NY, 1e30) == 0
    md.lit_reset(NX, NY)
    assert md.lit_status(NX, NY) == (0, TILES) and np.array_equal(md.lit_active_tiles(NX, NY), np.arange(TILES, dtype=np.int32))
    with pytest.raises(core.RtmiError) as e:
        md.lit_retire(NX, NY, 0.1)  # no samples yet: nothing to decide by
    assert e.value.code == E_STATE
    for s_count, exp in zip(ml.CHUNKS, want):
        _eq(md.lit_render(NX, NY, s_count, **_kw(MIS)), exp, "after reset")
    # a second frame object of another size on the same replicas leaves this one alone
    small = _single(scenes, MIS, ml.SMALL, (1, 3))
    _eq(md.lit_render(*ml.SMALL, 1, **_kw(MIS)), small[0], "a second frame")
    assert md.lit_status(NX, NY) == (8, TILES) and md.lit_status(*ml.SMALL) == (1, 4)


# ---- the same bytes however a call is split into sample passes ----------------------------------------------------------------------------------
def test_workspace_bytes_split_leaves_the_frame_unchanged(scenes, closing):
    """203 x 99 is 338 tiles, 169 per replica: 10 816 pixel slots of 5 samples of 24 bytes, 1.3 MB a call -- at the option's floor of 1 MiB every
    replica's call takes two passes (8 738 slots fit, 136 whole tiles), the second one partial"""
    size, chunks = fr.SIZE_PASSES["spheres"], (5, 5)
    assert ml.n_tiles(*size) == 338 and (1 << 20) // (5 * 24) // 64 == 136 < 169
    want = _single(scenes, MIS, size, chunks)
    md = _multi(closing, MIS, 2, options={"workspace_bytes": 1 << 20})
    for s_count, exp in zip(chunks, want):
        _eq(md.lit_render(*size, s_count, **_kw(MIS)), exp, "split passes")


# ---- the one-rank communicator path ------------------------------------------------------------------------------------------------------------
def test_rccl_gather_with_one_replica_equals_the_copy_path(scenes, closing, monkeypatch):
    if _ffi.lib().rtmi_rccl_probe(None) != 0:
        pytest.skip("no usable RCCL library on this host: " + _ffi.lib().rtmi_last_error().decode())
    want = _single(scenes, MIS)
    monkeypatch.setenv("RTMI_MULTI_GATHER", "rccl")
    forced = _multi(closing, MIS, 1)
    for s_count, exp in zip(ml.CHUNKS, want):
        _eq(forced.lit_render(NX, NY, s_count, **_kw(MIS)), exp, "rccl, one replica")
    assert forced.last_gather_path() == "rccl"
    two = _multi(closing, MIS, 2)
    with pytest.raises(core.RtmiError) as e:  # RCCL refuses one device twice: the gather policy, judged before anything is launched
        two.lit_render(NX, NY, 2, **_kw(MIS))
    assert e.value.code == E_ARG and "distinct devices" in str(e.value) and two.lit_status(NX, NY) == (0, TILES)
    monkeypatch.delenv("RTMI_MULTI_GATHER")
    _eq(two.lit_render(NX, NY, 1, **_kw(MIS)), want[0], "the copy path after the refusal")


# ---- distinct devices --------------------------------------------------------------------------------------------------------------------------
def test_two_distinct_devices(scenes, closing):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: the gather between devices needs two (the shared-device form is tested above)")
    want = _single(scenes, MIS)
    md = _multi(closing, MIS, 2, devices=[0, 1])
    for s_count, exp in zip(ml.CHUNKS, want):
        _eq(md.lit_render(NX, NY, s_count, **_kw(MIS)), exp, "two devices")
    assert md.last_gather_path() in ("rccl", "peer-copy")
    assert md.lit_retire(NX, NY, float(np.median(want[-1][2]))) < TILES


# ---- one process per GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [MIS, CONFIGS[8]], ids=["mis", "ris"])
def test_tile_renderer_step_lit_in_a_single_rank_world(scenes, closing, config):
    import torch
    md = _multi(closing, config, 2)
    tr = dist.TileRenderer(scenes(config[0], config[1]), NX, NY, 0, 1)
    kw = dict(estimator=config[2], light_choice=config[3], depth=DEPTH, seed=SEED)
    k = 0
    eps = None
    for s_count in ml.CHUNKS:
        exp = md.lit_render(NX, NY, s_count, **_kw(config))
        tr.step_lit(k, s_count, **kw)
        k += s_count
        torch.cuda.synchronize(_dev())
        got = (tr.linear.cpu().numpy(), tr.rgb8.cpu().numpy(), tr.stderr.cpu().numpy(), tr.samples.cpu().numpy(),
               tr.lit_counters.cpu().numpy().astype(np.uint64))
        _eq(got, exp, "step_lit k=%d" % k)
        if k == 4:  # retire about half of the tiles on both sides, by each side's own plane
            tx, ty = ml.tiles_xy(NX, NY)
            peaks = np.sort([np.max(exp[2][y * 8:y * 8 + 8, x * 8:x * 8 + 8]) for y in range(ty) for x in range(tx)])
            eps = float(0.5 * (peaks[7] + peaks[8]))
            left = md.lit_retire(NX, NY, eps)
            assert tr.retire_lit(eps) == left and 0 < left < TILES
            assert np.array_equal(tr.lit_tiles[:left].cpu().numpy(), md.lit_active_tiles(NX, NY))
    assert eps is not None and len(np.unique(got[3])) == 2
