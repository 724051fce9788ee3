"""rtmi_render_lit_tiles* and rtmi_tiles_retire*: light-sampled frames over a caller's list of 8x8 tiles, and the adaptive loop on top.

Every comparison is on bits.  The yardsticks are calls pinned elsewhere: rtmi_render_lit* / rtmi_render_lit_vol* of the whole frame (test_gpu_lit.py,
test_gpu_vol.py), rtmi_render_adaptive and rtmi_adaptive_retire (test_gpu_adaptive.py, test_gpu_adaptive_denoised.py); THE TILE ORDER and the retire
rule are lit_tiles_reference's (test_lit_tiles_host.py)."""

import numpy as np
import pytest

import adaptive_reference as ar
import depth_cases as dc
import frame_reference as fr
import lit_cases as lc
import lit_tiles_reference as ltr
from raytrace_clj_amd import _ffi, core
from tests import direct_cases as dcs
from tests import vol_cases as vcs

pytestmark = pytest.mark.gpu

bits = lc.bits
SEED = lc.SEED
POISON = -7.0
E_ARG, E_UNSUPPORTED, E_STATE = -1, -3, -5
PARTIAL = (21, 19, 2)  # 3 x 3 tiles, partial on both edges
DEPTH = 6


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    """(family, name) -> DeviceScene on the module's context, made once: "dc" depth_cases' scenes, "dcs" direct_cases', "vcs" vol_cases'"""
    made = {}
    flat = {"dc": dc.flat, "dcs": dcs.flat, "vcs": vcs.flat}

    def get(family, name):
        if (family, name) not in made:
            made[family, name] = core.DeviceScene(flat[family](name), ctx=ctx)
        return made[family, name]

    yield get
    for ds in made.values():
        ds.close()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _poisoned(nx, ny, rows=0, guard=0, state=True):
    """whole-frame HBM buffers and `rows` (+ `guard`) per-row outputs, all poison"""
    import torch
    full = lambda shape, v, dt=torch.float64: torch.full(shape, v, dtype=dt, device=_dev())  # noqa: E731
    d = dict(lin=full((ny, nx, 3), POISON), se=full((ny, nx), POISON), q=full((ny, nx, 3), 99, torch.uint8), cnt=full((4,), 9, torch.int64),
             state=full((nx * ny, _ffi.RAYS_REC), POISON) if state else None,
             rays=full((rows + guard, 3), POISON) if rows else None, cam=full((rows + guard, 8), POISON) if rows else None)
    torch.cuda.synchronize(_dev())
    return d


def _host(d):
    import torch
    torch.cuda.synchronize(_dev())
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


def _frame_call(ds, nx, ny, s_first, s_count, d, volume=False, stream=None, **kw):
    f = ds.render_lit_vol_device if volume else ds.render_lit_device
    f(nx, ny, s_first, s_count, d["lin"], d["se"], out_rgb8=d["q"], state=d["state"], out_rays=d["rays"], out_camera=d["cam"], out_counters=d["cnt"],
      stream=stream, **kw)


def _tiles_call(ds, nx, ny, s_first, s_count, tiles, d, volume=False, stream=None, **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(tiles, np.int32)).to(_dev())
    torch.cuda.synchronize(_dev())
    ds.render_lit_tiles_device(nx, ny, s_first, s_count, len(tiles), t, d["lin"], d["se"], d["q"], volume=volume, state=d["state"], out_rays=d["rays"],
                               out_camera=d["cam"], out_counters=d["cnt"], stream=stream, **kw)
    torch.cuda.synchronize(_dev())


def _same_bits(a, b, keys=("lin", "se", "q", "state")):
    return [k for k in keys if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


CONFIGS = [("dcs", "cornell", "plain", "f64", False, False), ("dcs", "cornell", "nee", "f64", False, False), ("dcs", "cornell", "mis", "f64", False, False),
           ("dcs", "sphere-lamp", "plain", "f64", False, False), ("dcs", "sphere-lamp", "nee", "f64", False, False),
           ("dcs", "sphere-lamp", "mis", "f64", False, False), ("dc", "cover", "plain", "f64", True, False), ("dc", "cover", "plain", "f32", False, False),
           ("vcs", "smoke", "mis", "f64", False, True)]


# ---- 1. all tiles = the frame ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.SHAPES + (PARTIAL,))
@pytest.mark.parametrize("family, name, estimator, precision, lens, volume", CONFIGS)
def test_all_tiles_are_the_frame(ctx, scenes, family, name, estimator, precision, lens, volume, shape):
    nx, ny, ns = shape
    every = ltr.all_tiles(nx, ny)
    rows = len(every) * 64 * ns
    if lens:  # the scene's own thin lens opened to a real width (test_gpu_lit._lens): the disk point moves the ray
        f = dc.flat(name)
        cam = np.array(f.cam, np.float64)
        assert int(f.cam_kind) == 1 and cam[21] == 0.0
        cam[21] = 0.3
        ds = core.DeviceScene(f, ctx=ctx)
        ds.set_camera((1, cam))
    else:
        ds = scenes(family, name)
    kw = dict(estimator=estimator, depth=DEPTH, seed=SEED, precision=precision)
    try:
        want, got = _poisoned(nx, ny, nx * ny * ns), _poisoned(nx, ny, rows)
        _frame_call(ds, nx, ny, 0, ns, want, volume, **kw)
        _tiles_call(ds, nx, ny, 0, ns, every, got, volume, **kw)
    finally:
        if lens:
            ds.close()
    want, got = _host(want), _host(got)
    what = (name, estimator, precision, lens, volume, shape)
    assert _same_bits(got, want) == [], what
    assert got["cnt"].tolist() == want["cnt"].tolist() and got["cnt"][1] == nx * ny * ns and (got["cnt"][2] > 0) == (estimator != "plain"), (what, got["cnt"])
    has, frame_row = ltr.frame_rows(nx, ny, 0, ns, every)
    for k in ("rays", "cam"):
        assert np.array_equal(bits(got[k][has]), bits(want[k][frame_row])), (what, k)
        assert (bits(got[k][~has]) == 0).all(), (what, k, "rows without a pixel are +0.0")
    assert (~has).sum() == rows - nx * ny * ns and (want["state"][:, 9] == ns).all()


# ---- 2. a prescribed schedule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family, name, estimator, volume", [("dcs", "cornell", "nee", False), ("dcs", "cornell", "mis", False), ("vcs", "smoke", "mis", True)])
def test_a_prescribed_schedule_leaves_every_tile_at_its_own_frame(scenes, family, name, estimator, volume):
    """21 x 19, three rounds of 2 samples.  Round 1 lists every tile, round 2 the tiles with t % 3 != 1, round 3 the right-column and bottom-row tiles
    among those (a tile that sat out round 2 cannot take samples [4, 6): its state holds 2), so the tiles end with 2, 4 and 6 samples and the corner
    tiles, partial on one or both edges, with 6.  Afterwards every pixel is the frame call's at ns = what its tile took; a tile absent from a round
    keeps every bit across it, in all four in/out buffers."""
    nx, ny, n = PARTIAL
    tx, ty = ltr.tiles_of(nx, ny)
    every = ltr.all_tiles(nx, ny)
    second = every[every % 3 != 1]
    edge = every[(every % tx == tx - 1) | (every // tx == ty - 1)]
    lists = [every, second, np.intersect1d(second, edge)]
    assert [len(t) for t in lists] == [9, 6, 4] and set(edge) - set(second) == {7}
    ds = scenes(family, name)
    kw = dict(estimator=estimator, depth=DEPTH, seed=SEED)
    frames, d = {}, _poisoned(nx, ny)
    for r in range(3):  # the yardstick: the frame call refined through one state, a snapshot after every chunk
        _frame_call(ds, nx, ny, r * n, n, d, volume, **kw)
        frames[(r + 1) * n] = _host(d)
    got = _poisoned(nx, ny)
    took = np.zeros((ny, nx), np.int64)
    total = np.zeros(4, np.int64)
    for r, tiles in enumerate(lists):
        before = _host(got)
        _tiles_call(ds, nx, ny, r * n, n, tiles, got, volume, **kw)
        after = _host(got)
        on = ltr.pixel_mask(nx, ny, tiles)
        took[on] += n
        for k, a, b in (("lin", after["lin"], before["lin"]), ("q", after["q"], before["q"]), ("se", after["se"], before["se"]),
                        ("state", after["state"].reshape(ny, nx, -1), before["state"].reshape(ny, nx, -1))):
            assert np.array_equal(a[~on].view(np.uint8), b[~on].view(np.uint8)), (r, k, "an unlisted tile changed")
        assert after["cnt"][1] == on.sum() * n and after["cnt"][2] > 0, (r, after["cnt"])
        total += after["cnt"]
    assert sorted(np.unique(took).tolist()) == [2, 4, 6]
    for level in (2, 4, 6):
        m, want = took == level, frames[level]
        assert m.any()
        for k in ("lin", "q", "se"):
            assert np.array_equal(after[k][m].view(np.uint8), want[k][m].view(np.uint8)), (level, k)
        assert np.array_equal(after["state"].reshape(ny, nx, -1)[m].view(np.uint8), want["state"].reshape(ny, nx, -1)[m].view(np.uint8)), (level, "state")
    assert (after["state"][:, 9].reshape(ny, nx) == took).all() and total[1] == took.sum()


# ---- 3. the closed loop against the adaptive frame ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ar.CASES[0], ar.CASES[2]], ids=ar.case_id)
def test_the_closed_loop_is_the_adaptive_frame(ctx, case):
    name, precision, (nx, ny), first, chunk, cap, eps = case
    ds = core.DeviceScene(fr.scene(name, nx, ny), ctx=ctx)
    try:
        want, lists = [], []
        try:
            for g in ds.refine_adaptive(nx, ny, cap, chunk, eps, first=first, precision=precision, depth=fr.DEPTH, seed=fr.SEED):
                want.append(g)
                lists.append(ctx.adaptive_active_tiles())
        finally:
            ctx.progressive_release()
        lin, q, err, smp, cnt, rounds = ds.refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, estimator="plain", precision=precision, depth=fr.DEPTH,
                                                               seed=fr.SEED)
        assert ctx.progressive_samples() == 0
    finally:
        ds.close()
    assert [k for k, _ in rounds] == [g[0] for g in want]
    for (k, tiles), adaptive_list in zip(rounds, lists):
        assert tiles.dtype == np.int32 and np.array_equal(tiles, adaptive_list), (k, "the list after the round")
    sizes = [len(ltr.all_tiles(nx, ny))] + [len(t) for _, t in rounds]
    shrank = [i for i in range(1, len(sizes)) if sizes[i] < sizes[i - 1]]
    assert len(shrank) >= 2 and sizes[1] > 0, "void: the case must retire tiles in at least two rounds and keep some after the first (%r)" % (sizes,)
    k, wlin, wq, werr, wsmp, wcnt, _ = want[-1]
    assert np.array_equal(bits(lin), bits(wlin)) and np.array_equal(q, wq) and np.array_equal(bits(err), bits(werr))
    assert smp.dtype == np.int32 and np.array_equal(smp, wsmp) and len(np.unique(smp)) >= 2
    assert int(cnt[0]) == int(wcnt[0]) and int(cnt[1]) == int(smp.sum()) and cnt.tolist()[2:] == [0, 0]


def test_the_denoised_loop_retires_on_the_filtered_error(scenes):
    nx, ny = 40, 24
    ds = scenes("dcs", "cornell")
    kw = dict(estimator="mis", depth=DEPTH, seed=SEED)
    lin, q, err, smp, cnt, rounds = ds.refine_lit_adaptive(nx, ny, 12, 4, 0.05, denoised=True, **kw)
    # the same rounds by hand on the host forms: features once, then trace, filter, retire
    ft = ds.render_features(nx, ny, core.FEATURE_SAMPLES, SEED)[0]
    hl, hq, he = np.zeros((ny, nx, 3)), np.zeros((ny, nx, 3), np.uint8), np.zeros((ny, nx))
    state, tiles, k = np.zeros((nx * ny, _ffi.RAYS_REC)), ltr.all_tiles(nx, ny), 0
    for kk, listed in rounds:
        ds.render_lit_tiles(nx, ny, k, kk - k, tiles, hl, hq, he, state, **kw)
        tiles = ds.ctx.tiles_retire(ds.ctx.denoise(hl, he, ft)[2], 0.05, tiles)
        assert np.array_equal(tiles, listed), kk
        k = kk
    assert np.array_equal(bits(hl), bits(lin)) and np.array_equal(hq, q) and np.array_equal(bits(he), bits(err))
    assert np.array_equal(state[:, 9].reshape(ny, nx).astype(np.int32), smp) and (k == 12 or len(tiles) == 0)


# ---- 4. tiles_retire on the device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ltr.RETIRE_SHAPES)
def test_tiles_retire_is_the_reference_rule(ctx, shape):
    import torch
    nx, ny = shape
    every = ltr.all_tiles(nx, ny)
    for name, noise, eps in ltr.retire_maps(nx, ny):
        for tiles in (every, every[::2], every[::-1].copy()):
            want = ltr.retire(noise, eps, tiles)
            assert np.array_equal(ctx.tiles_retire(noise, eps, tiles), want), (name, "host form")
            d_noise = torch.from_numpy(noise).to(_dev())
            for aliased in (True, False):
                t_in = torch.from_numpy(np.ascontiguousarray(tiles)).to(_dev())
                t_out = None if aliased else torch.full((len(tiles) + 3,), -5, dtype=torch.int32, device=_dev())
                torch.cuda.synchronize(_dev())
                n = ctx.tiles_retire_device(nx, ny, d_noise, eps, len(tiles), t_in, t_out)
                torch.cuda.synchronize(_dev())
                out = (t_in if aliased else t_out).cpu().numpy()
                assert n == len(want) and np.array_equal(out[:n], want), (name, aliased)
                if aliased:
                    assert np.array_equal(out[n:], tiles[n:]), (name, "entries behind the survivors keep what they held")
                else:
                    assert (out[n:] == -5).all() and np.array_equal(t_in.cpu().numpy(), tiles), (name, "nothing else is written")


def test_tiles_retire_retires_what_adaptive_retire_retires(ctx, scenes):
    nx, ny = 61, 37
    ds = scenes("dcs", "cornell")
    try:
        err = ds.render_progressive(nx, ny, 0, 8, DEPTH, SEED)[2]
        worst = np.unique(ar.tile_max(err))
        eps = float(worst[len(worst) // 2])  # an exact tie at a tile's own maximum: that tile retires
        retired = ctx.adaptive_retire(err, eps)
        left = ctx.adaptive_active_tiles()
    finally:
        ctx.progressive_release()
    every = ltr.all_tiles(nx, ny)
    assert 0 < retired < len(every) and len(left) == len(every) - retired
    assert np.array_equal(ctx.tiles_retire(err, eps, every), left) and np.array_equal(ltr.retire(err, eps, every), left)
    assert ctx.progressive_samples() == 0


# ---- 5. passes and forms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (PARTIAL, (21, 19, 350)))
def test_workspace_passes_of_whole_tiles_change_no_bit(ctx, scenes, shape):
    """without out_rays the radiance lives in the workspace.  Option "workspace_bytes" has a floor of 1 MiB, which holds one tile of 64 x s_count x 24
    bytes per pass only from 342 samples on: 21 x 19 x 2 (nine tiles in one pass at the floor) is run for the record, 21 x 19 x 350 takes nine passes
    of one tile each -- every pass but the first starts at a later entry of the list"""
    nx, ny, ns = shape
    every = ltr.all_tiles(nx, ny)
    per_pass = max(1, (1 << 20) // (ns * 24) // 64)
    assert per_pass == (1 if ns == 350 else 341)
    ds = scenes("dcs", "cornell")
    outs = []
    try:
        for ws in (1 << 20, 64 << 30):
            ctx.set_option("workspace_bytes", ws)
            d = _poisoned(nx, ny)
            d["cam"] = _poisoned(1, 1, len(every) * 64 * ns)["cam"]
            _tiles_call(ds, nx, ny, 0, ns, every, d, estimator="mis", depth=3, seed=SEED)
            outs.append(_host(d))
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
    assert _same_bits(outs[0], outs[1], ("lin", "se", "q", "state", "cam")) == [] and outs[0]["cnt"].tolist() == outs[1]["cnt"].tolist()
    assert outs[0]["cnt"][1] == nx * ny * ns and outs[0]["cnt"][2] > 0 and (outs[0]["lin"] != POISON).all()


def test_device_form_on_the_callers_stream_is_the_host_form(ctx, scenes):
    import torch
    nx, ny, ns = PARTIAL
    ds = scenes("dcs", "cornell")
    every = ltr.all_tiles(nx, ny)
    tiles = every[every % 3 != 1]
    kw = dict(estimator="mis", light_choice="power", depth=DEPTH, seed=SEED)
    lin, q, se = np.full((ny, nx, 3), POISON), np.full((ny, nx, 3), 99, np.uint8), np.full((ny, nx), POISON)
    state = np.full((nx * ny, _ffi.RAYS_REC), POISON)
    cnt, rays, cam = ds.render_lit_tiles(nx, ny, 0, ns, tiles, lin, q, se, state, return_rays=True, return_camera=True, **kw)
    try:
        ds.render_progressive(nx, ny, 0, 2, DEPTH, SEED)
        stream = torch.cuda.Stream(_dev())
        d = _poisoned(nx, ny, len(tiles) * 64 * ns)
        _tiles_call(ds, nx, ny, 0, ns, tiles, d, stream=stream.cuda_stream, **kw)
        assert ctx.progressive_samples() == 2
    finally:
        ctx.progressive_release()
    got = _host(d)
    for k, want in (("lin", lin), ("q", q), ("se", se), ("state", state), ("rays", rays.reshape(-1, 3)), ("cam", cam.reshape(-1, 8))):
        assert np.array_equal(got[k].view(np.uint8), want.view(np.uint8)), k
    assert got["cnt"].tolist() == cnt.tolist()
    on = ltr.pixel_mask(nx, ny, tiles)
    assert (lin[~on] == POISON).all() and (lin[on] != POISON).all() and (q[~on] == 99).all() and (se[~on] == POISON).all()
    assert (state.reshape(ny, nx, -1)[~on] == POISON).all() and (state.reshape(ny, nx, -1)[on][:, 9] == ns).all()


def test_a_device_list_entry_outside_the_frame_holds_no_pixel(scenes):
    """a bounds guard checked by its effect: entries -1, T and 2^31 - 1 among valid ones give the valid entries' result and nothing else is written --
    not in the frame, not in the state, not in their own rows of out_rays / out_camera, not behind the last row"""
    nx, ny, ns = PARTIAL
    ds = scenes("dcs", "cornell")
    n_all = len(ltr.all_tiles(nx, ny))
    valid = np.array([0, 5, 8], np.int32)
    mixed = np.array([-1, 0, n_all, 5, 2 ** 31 - 1, 8], np.int32)
    kw = dict(estimator="mis", depth=DEPTH, seed=SEED)
    guard, block = 64, 64 * ns
    want, got = _poisoned(nx, ny, len(valid) * block), _poisoned(nx, ny, len(mixed) * block, guard)
    _tiles_call(ds, nx, ny, 0, ns, valid, want, **kw)
    _tiles_call(ds, nx, ny, 0, ns, mixed, got, **kw)
    want, got = _host(want), _host(got)
    assert _same_bits(got, want) == [] and got["cnt"].tolist() == want["cnt"].tolist()
    on = ltr.pixel_mask(nx, ny, valid)
    assert (got["lin"][~on] == POISON).all() and (got["se"][~on] == POISON).all() and (got["q"][~on] == 99).all()
    assert (got["state"].reshape(ny, nx, -1)[~on] == POISON).all()
    for k in ("rays", "cam"):
        for i, t in enumerate(mixed):
            rows = got[k][i * block:(i + 1) * block]
            if t in valid:
                j = int(np.flatnonzero(valid == t)[0])
                assert np.array_equal(bits(rows), bits(want[k][j * block:(j + 1) * block])), (k, t)
            else:
                assert (rows == POISON).all(), (k, t)
        assert (got[k][len(mixed) * block:] == POISON).all(), (k, "behind the last row")


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_headers_order_launch_nothing(ctx, scenes):
    L, p = _ffi.lib(), core.ptr
    ds, smoke = scenes("dcs", "sphere-lamp"), scenes("vcs", "smoke")
    nx, ny = 13, 7
    lin, se, q = np.full((ny, nx, 3), POISON), np.full((ny, nx), POISON), np.full((ny, nx, 3), 99, np.uint8)
    cnt, state = np.full(4, 9, np.uint64), np.full((nx * ny, _ffi.RAYS_REC), POISON)
    tiles, many = np.array([0, 1], np.int32), np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)
    err = lambda: L.rtmi_last_error().decode()  # noqa: E731

    def call(scene, s_first=0, s_count=1, estimator=2, n_lights=0, prims=None, choice=0, precision=0, volume=0, n_tiles=2, tl=tiles, out=lin, st=None):
        return L.rtmi_render_lit_tiles(scene.handle, precision, nx, ny, s_first, s_count, 5, 1, estimator, n_lights, p(prims), choice, volume, n_tiles, p(tl),
                                       p(st), p(out), p(q), p(se), None, None, p(cnt))
    late = dict(precision=7, n_lights=len(many), prims=many, choice=5)  # what is reported later never hides what is reported first
    assert call(ds, s_count=0, estimator=9, volume=7, n_tiles=-1, **late) == E_ARG and "s_count" in err()
    assert call(ds, estimator=9, volume=7, n_tiles=-1, out=None, **late) == E_ARG and "NULL" in err()
    assert call(ds, estimator=9, volume=7, n_tiles=-1, **late) == E_ARG and "estimator" in err()
    assert call(ds, volume=7, n_tiles=-1, **late) == E_ARG and "volume" in err()
    assert call(ds, n_tiles=-1, tl=np.array([5], np.int32), **late) == E_ARG and "n_tiles" in err()
    assert call(ds, tl=None, **late) == E_ARG and "n_tiles" in err()
    assert call(ds, tl=np.array([0, 2], np.int32), **late) == E_ARG and "tiles[1]" in err()
    assert call(ds, tl=np.array([1, 0], np.int32), **late) == E_ARG and "ascending" in err()
    assert call(ds, **late) == E_ARG and "precision" in err()
    assert call(smoke, **dict(late, precision=1)) == E_UNSUPPORTED                        # RTMI_F32 on a mixed-kind scene, as rtmi_render_lit
    assert call(ds, **dict(late, precision=0)) == E_ARG and "n_lights" in err()
    assert call(ds, volume=1, estimator=0) == E_ARG and "estimator" in err()               # the volume rule takes estimators 1 and 2
    assert call(ds, choice=5) == E_ARG and "light_choice" in err()
    assert call(smoke) == E_UNSUPPORTED and "ConstantMedium" in err()                       # volume 0 keeps rtmi_render_lit's refusal of media
    assert call(ds, n_lights=1, prims=np.array([10 ** 6], np.int32)) == E_ARG
    held = np.zeros_like(state)
    held[:, 9] = 3
    held[(ny - 1) * nx + nx - 1, 9] = 2  # the last pixel of the image: in tile 1
    before = held.copy()
    assert call(ds, s_first=3, st=held) == E_STATE and "tile 1" in err()
    assert np.array_equal(held, before)
    assert (lin == POISON).all() and (se == POISON).all() and (q == 99).all() and (cnt == 9).all() and (state == POISON).all()
    # ... and the calls that must succeed: an empty list launches nothing; a pixel outside the list may hold any count
    assert call(ds, n_tiles=0, tl=None) == 0 and (lin == POISON).all() and (cnt == 9).all()
    assert call(ds, s_first=3, st=held, n_tiles=1) == 0 and cnt[1] == 8 * ny and (held[:8, 9] == 4).all() and held[(ny - 1) * nx + nx - 1, 9] == 2
    assert call(smoke, volume=1) == 0 and cnt[1] == nx * ny and cnt[2] > 0 and (lin != POISON).all()
    with pytest.raises(ValueError):
        ds.render_lit_tiles(nx, ny, 0, 1, tiles, lin[:, :, 0], q, se)
    with pytest.raises(ValueError):
        ds.render_lit_tiles(nx, ny, 0, 1, tiles, lin, q, se, estimator="bdpt")


# ---- 7. the command line --------------------------------------------------------------------------------------------------------------------------
def test_cli_lit_adaptive_writes_refine_lit_adaptives_frame(tmp_path, capsys):
    from raytrace_clj_amd import scene as scenes_module
    name = str(tmp_path / "box.npy")
    assert core.main([name, "21", "19", "12", "cornell-box-classic", "--lit", "mis", "--adaptive", "0.08", "--chunk", "4"]) == 0
    lit = np.load(str(tmp_path / "box.lit.npy"))
    said = capsys.readouterr().out
    ds = core.DeviceScene(core.SCENES["cornell-box-classic"](scenes_module, 21, 19))
    try:
        _, want, _, smp, _, rounds = ds.refine_lit_adaptive(21, 19, 12, 4, 0.08, estimator="mis")
        uniform = ds.render_lit(21, 19, 12, estimator="mis")[1]
    finally:
        ds.close()
    assert np.array_equal(lit, want)
    share = 100.0 * float(smp.sum()) / (21 * 19 * 12)
    assert ("--lit: %.1f%% of the %d pixel-samples taken" % (share, 21 * 19 * 12)) in said
    assert len(rounds) >= 1 and (share == 100.0 or not np.array_equal(lit, uniform))
