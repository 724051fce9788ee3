"""rtmi_render_lit*: light-sampled frames of the scene's own camera, the rays built on the device.

Every comparison is on bits.  The yardsticks are the device's own calls, pinned elsewhere: estimator 0 must be the frame of rtmi_render and
rtmi_render_progressive; the camera rays must be depth_cases.frame_paths' (lit_cases.frame_groups; test_lit_host.py ties that chain to the oracle's
frame); every row's radiance must be rtmi_probe_paths_nee / _mis of the call's own camera ray from the stream position the camera left; the frame
must be rays_reference.fold of those rows; and chunks, workspace passes, live edits and the device form must change no bit."""
import numpy as np
import pytest

import depth_cases as dc
import lit_cases as lc
import rays_reference as rr
from raytrace_clj_amd import _ffi, core
from tests import direct_cases as dcs
from tests import mis_cases as mcs
from tests import nee_cases as ncs

pytestmark = pytest.mark.gpu

bits = lc.bits
SEED = lc.SEED


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx):
    """(family, name) -> DeviceScene on the module's context, made once: "dc" names depth_cases' scenes, "dcs" direct_cases'"""
    made = {}

    def get(family, name):
        if (family, name) not in made:
            made[family, name] = core.DeviceScene((dc.flat if family == "dc" else dcs.flat)(name), ctx=ctx)
        return made[family, name]

    yield get
    for ds in made.values():
        ds.close()


def _lens(f, aperture=0.3):
    """the scene's own thin lens opened to a real width: the disk point now moves the ray"""
    cam = np.array(f.cam, np.float64)
    assert int(f.cam_kind) == 1 and cam[21] == 0.0
    cam[21] = aperture
    return 1, cam


def _dev():
    import torch
    return torch.device("cuda", 0)


def _device_call(ds, nx, ny, s_first, s_count, state=None, want_rays=True, want_camera=False, stream=None, **kw):
    """one render_lit_device call into poison-filled HBM buffers -> dict of host arrays"""
    import torch
    npx, n = nx * ny, nx * ny * s_count
    full = lambda shape, v, dt=torch.float64: torch.full(shape, v, dtype=dt, device=_dev())
    d = dict(lin=full((ny, nx, 3), -7.0), se=full((ny, nx), -7.0), q=full((ny, nx, 3), 99, torch.uint8), cnt=full((4,), 9, torch.int64),
             rays=full((n, 3), -7.0) if want_rays else None, cam=full((n, 8), -7.0) if want_camera else None,
             state=torch.from_numpy(state).to(_dev()) if state is not None else None)
    torch.cuda.synchronize(_dev())
    ds.render_lit_device(nx, ny, s_first, s_count, d["lin"], d["se"], out_rgb8=d["q"], state=d["state"], out_rays=d["rays"], out_camera=d["cam"],
                         out_counters=d["cnt"], stream=stream, **kw)
    torch.cuda.synchronize(_dev())
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


# ---- 1. estimator 0 is the frame ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.SHAPES)
@pytest.mark.parametrize("name, precision, lens", [("cover", "f64", False), ("cover", "f64", True), ("cornell", "f64", False),
                                                   ("hitlist-media", "f64", False), ("cover", "f32", False)])
def test_estimator_0_is_the_frame(ctx, name, precision, lens, shape):
    nx, ny, ns = shape
    f = dc.flat(name)
    ds = core.DeviceScene(f, ctx=ctx)
    try:
        if lens:
            assert ds.set_camera(_lens(f)) is False
        lin, q, err, cnt = ds.render_lit(nx, ny, ns, estimator="plain", depth=dc.FULL, seed=SEED, precision=precision)
        flin, fq, fcnt = ds.render(nx, ny, ns, dc.FULL, SEED, precision)
        try:
            plin, pq, perr, pcnt = ds.render_progressive(nx, ny, 0, ns, dc.FULL, SEED, precision)
        finally:
            ctx.progressive_release()
    finally:
        ds.close()
    what = (name, precision, lens, shape)
    assert np.array_equal(bits(lin), bits(flin)), (what, "%d pixels differ from render's" % (lin != flin).any(axis=2).sum())
    assert np.array_equal(q, fq) and int(cnt[0]) == int(fcnt[0]) and cnt.tolist()[1:] == [nx * ny * ns, 0, 0], (what, cnt, fcnt)
    assert np.array_equal(bits(plin), bits(lin)) and np.array_equal(pq, q) and np.array_equal(bits(perr), bits(err)) and int(pcnt[0]) == int(cnt[0]), what
    assert np.isfinite(err).all() and (err > 0).any()
    if precision == "f32":
        assert np.array_equal(lin.astype(np.float32).astype(np.float64), lin)


# ---- 2. the camera rays ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.SHAPES)
@pytest.mark.parametrize("name", ("cover", "cornell"))
def test_out_camera_is_the_frames_rays(scenes, oracle, name, shape):
    nx, ny, ns = shape
    f = dc.flat(name)
    cam = scenes("dc", name).render_lit(nx, ny, ns, estimator="plain", depth=0, seed=SEED, return_camera=True)[4].reshape(-1, 8)
    rays, keys, ctr = lc.frame_groups(lambda uv, k: oracle.probe_camera(f, uv, k), f, nx, ny, ns, SEED)
    assert np.array_equal(bits(cam[:, :7]), bits(rays)), "%d of %d rays differ" % ((bits(cam[:, :7]) != bits(rays)).any(axis=1).sum(), len(rays))
    assert np.array_equal(cam[:, 7], ctr.astype(np.float64)) and len(np.unique(ctr)) > 1
    assert np.array_equal(keys, lc.frame_keys(nx, ny, ns, SEED))
    # samples [1, 3) alone: the same rays, the keys offset by s_first
    part = _device_call(scenes("dc", name), nx, ny, 1, 2, want_camera=True, estimator="plain", depth=0, seed=SEED)["cam"]
    want = lc.frame_groups(lambda uv, k: oracle.probe_camera(f, uv, k), f, nx, ny, 2, SEED, s_first=1)
    assert np.array_equal(bits(part[:, :7]), bits(want[0])) and np.array_equal(part[:, 7], want[2].astype(np.float64))


# ---- 3. per-ray radiance, the fold, the counters --------------------------------------------------------------------------------------------------------
def _check_rows(ds, f, nx, ny, ns, depth, precision, what):
    keys = lc.frame_keys(nx, ny, ns, SEED)
    max_seg = depth + 1
    seen = 0
    for estimator, choice in (("nee", 0), ("mis", 0), ("mis", 1)):
        lin, q, err, cnt, out, cam = ds.render_lit(nx, ny, ns, estimator=estimator, light_choice=choice, depth=depth, seed=SEED, precision=precision,
                                                   return_rays=True, return_camera=True)
        out, cam = out.reshape(-1, 3), cam.reshape(-1, 8)
        if estimator == "nee":
            probe = lambda r, k, ctr0: ds.probe_paths_nee(r, k, depth=depth, ctr0=ctr0, max_seg=max_seg, precision=precision)
        else:
            probe = lambda r, k, ctr0: ds.probe_paths_mis(r, k, light_choice=choice, depth=depth, ctr0=ctr0, max_seg=max_seg, precision=precision)
        rgb, nseg, log, nlog, _ = lc.probe_by_ctr(probe, np.ascontiguousarray(cam[:, :7]), keys, cam[:, 7])
        w = (what, estimator, choice)
        assert np.array_equal(bits(out), bits(rgb)), (w, "%d of %d rows differ from the probe's" % ((bits(out) != bits(rgb)).any(axis=1).sum(), len(out)))
        state = log[:, :, 12]
        want = [int(nseg.sum()), nx * ny * ns, int(((state == 1.0) | (state == 2.0)).sum()), int((state == 2.0).sum())]
        assert cnt.tolist() == want, (w, cnt, want)
        elin, eerr = lc.folded_frame(out, nx, ny, ns, precision)
        assert np.array_equal(bits(lin), bits(elin)) and np.array_equal(bits(err), bits(eerr)), w
        assert np.array_equal(q, ds.ctx.denoise(lin, iterations=0)[1]), w
        seen += want[2]
    return seen


@pytest.mark.parametrize("depth", ncs.DEPTHS)
@pytest.mark.parametrize("name, precision", ncs.CASES)
def test_every_row_is_the_probes_path(scenes, name, precision, depth):
    nx, ny, ns = lc.SMALL
    built = _check_rows(scenes("dcs", name), dcs.flat(name), nx, ny, ns, depth, precision, (name, precision, depth))
    assert (built > 0) == (depth > 0)  # no scatter at depth 0, no light sample


def test_every_row_is_the_probes_path_through_a_real_lens(ctx):
    nx, ny, ns = lc.SMALL
    f = dcs.flat("sphere-lamp")
    ds = core.DeviceScene(f, ctx=ctx)
    try:
        ds.set_camera(_lens(f))
        cam = ds.render_lit(nx, ny, ns, estimator="plain", depth=0, seed=SEED, return_camera=True)[4].reshape(-1, 8)
        assert len(np.unique(bits(cam[:, 0]))) > nx * ny and len(np.unique(cam[:, 6])) > nx * ny  # origins on the lens, times in the shutter
        assert _check_rows(ds, f, nx, ny, ns, 3, "f64", "lens") > 0
    finally:
        ds.close()


# ---- 4. chunks ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, precision", (("cornell", "f64"), ("sphere-lamp", "f32")))
def test_chunks_with_a_state_are_the_one_shot(scenes, name, precision):
    nx, ny, _ = lc.SMALL
    ds = scenes("dcs", name)
    kw = dict(estimator="mis", light_choice=1, depth=8, seed=SEED, precision=precision)
    one = _device_call(ds, nx, ny, 0, 5, state=rr.new_state(nx * ny), **kw)
    a = _device_call(ds, nx, ny, 0, 2, state=rr.new_state(nx * ny), **kw)
    b = _device_call(ds, nx, ny, 2, 3, state=a["state"], **kw)
    for k in ("lin", "se", "q", "state"):
        assert np.array_equal(b[k], one[k]) and (k == "q" or np.array_equal(bits(b[k]), bits(one[k]))), k
    assert (a["cnt"] + b["cnt"]).tolist() == one["cnt"].tolist() and one["cnt"][1] == nx * ny * 5 and one["cnt"][2] > one["cnt"][3] > 0
    assert (one["state"][:, 9] == 5).all()
    # without a state s_first only offsets the keys: rows 2..4 of the one-shot, folded on their own
    alone = _device_call(ds, nx, ny, 2, 3, **kw)
    rows = one["rays"].reshape(nx * ny, 5, 3)[:, 2:]
    assert np.array_equal(bits(alone["rays"]), bits(rows.reshape(-1, 3))) and np.array_equal(bits(alone["rays"]), bits(b["rays"]))
    elin, eerr = lc.folded_frame(alone["rays"], nx, ny, 3, precision)
    assert np.array_equal(bits(alone["lin"]), bits(elin)) and np.array_equal(bits(alone["se"]), bits(eerr))
    assert not np.array_equal(bits(alone["lin"]), bits(one["lin"]))


# ---- 5. workspace passes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", ("plain", "mis"))
def test_workspace_passes_change_no_bit(ctx, scenes, estimator):
    """without out_rays the radiance lives in the workspace: at its floor of 1 MiB a 40 x 24 x 100 frame (2.3 MB of samples) takes three passes of 436,
    436 and 88 pixels -- 436 = 10 rows and 36 pixels, so both boundaries fall inside an image row and row0 enters every later pass's pixels and keys"""
    nx, ny, ns = 40, 24, 100
    per_pass = (1 << 20) // (ns * 24)
    assert -(-nx * ny // per_pass) >= 3 and per_pass % nx != 0 and (2 * per_pass) % nx != 0
    ds = scenes("dcs", "sphere-lamp")
    outs = []
    try:
        for ws in (1 << 20, 64 << 30):
            ctx.set_option("workspace_bytes", ws)
            outs.append(_device_call(ds, nx, ny, 3, ns, want_rays=False, want_camera=True, estimator=estimator, depth=4, seed=SEED))
    finally:
        ctx.set_option("workspace_bytes", 64 << 30)
    for k in ("lin", "se", "q", "cam", "cnt"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert np.array_equal(bits(outs[0]["lin"]), bits(outs[1]["lin"])) and np.array_equal(bits(outs[0]["cam"]), bits(outs[1]["cam"]))
    assert outs[0]["cnt"][1] == nx * ny * ns and (outs[0]["cam"] != -7.0).all() and (outs[0]["cnt"][2] > 0) == (estimator == "mis")


# ---- 6. live edits ------------------------------------------------------------------------------------------------------------------------------------
def test_a_moved_camera_is_the_fresh_scenes_view(ctx):
    import torch
    nx, ny, ns = lc.SMALL
    f = dcs.flat("sphere-lamp")
    moved = core.DeviceScene(dcs.sphere_lamp_scene(), ctx=ctx)
    views = [_lens(f), (1, np.array(dcs.flat("example-light").cam, np.float64))]
    kw = dict(estimator="mis", depth=6, seed=SEED)
    try:
        before = _device_call(moved, nx, ny, 0, ns, want_camera=True, **kw)
        stream = torch.cuda.Stream(_dev())
        for k, view in enumerate(views):
            import copy
            g = copy.copy(f)
            g.cam_kind, g.cam = view
            fresh = core.DeviceScene(g, ctx=ctx)
            try:
                want = _device_call(fresh, nx, ny, 0, ns, want_camera=True, **kw)
            finally:
                fresh.close()
            if k == 0:
                moved.set_camera(view)
                got = _device_call(moved, nx, ny, 0, ns, want_camera=True, **kw)
            else:  # in stream order on the caller's stream: the camera kernel, then the frame
                moved.set_camera(view, stream=stream)
                got = _device_call(moved, nx, ny, 0, ns, want_camera=True, stream=stream.cuda_stream, **kw)
            for key in ("lin", "se", "q", "rays", "cam", "cnt"):
                assert np.array_equal(got[key], want[key]), (k, key)
            assert np.array_equal(bits(got["rays"]), bits(want["rays"])) and not np.array_equal(bits(got["cam"]), bits(before["cam"]))
    finally:
        moved.close()


def test_a_lamp_switched_off_is_no_longer_sampled(ctx):
    """the rectangle lamp's emission set to zero by a material edit: picked by power it has no weight, so the frame is the one that lists the other
    lamp alone -- the same light samples, the same shares -- and it is the frame of a scene created dark"""
    nx, ny, ns = lc.SMALL
    lit, dark = mcs.two_lamp_flat(), mcs.two_lamp_flat((0.0, 0.0, 0.0))
    ds = core.DeviceScene(lit, ctx=ctx)
    fresh = core.DeviceScene(dark, ctx=ctx)
    kw = dict(estimator="mis", light_choice="power", depth=6, seed=SEED, return_rays=True)
    try:
        lights = ds.lights().tolist()
        assert len(lights) == 2
        before = ds.render_lit(nx, ny, ns, **kw)
        ds.set_materials(dark)
        after = ds.render_lit(nx, ny, ns, **kw)
        want = fresh.render_lit(nx, ny, ns, **kw)
        off = [p for p in lights if not _emits(dark, p)]
        assert len(off) == 1
        alone = ds.render_lit(nx, ny, ns, lights=[p for p in lights if p != off[0]], **kw)
    finally:
        ds.close(); fresh.close()
    for a, b in zip(after, want):
        assert np.array_equal(a, b)
    assert np.array_equal(bits(after[4]), bits(alone[4])) and after[3].tolist() == alone[3].tolist() and np.array_equal(bits(after[0]), bits(alone[0]))
    assert not np.array_equal(bits(after[4]), bits(before[4])) and after[3][2] > 0


def _emits(f, prim):
    from raytrace_clj_amd import camera
    table = camera.light_table(f, np.array([prim], np.int32))
    return bool(table[0, 7:10].any())


# ---- 7. the device form -------------------------------------------------------------------------------------------------------------------------------
def test_device_form_on_the_callers_stream_leaves_the_progressive_frame_alone(ctx, scenes):
    import torch
    nx, ny, ns = lc.SMALL
    ds = scenes("dcs", "cornell")
    kw = dict(estimator="mis", depth=6, seed=SEED)
    host = ds.render_lit(nx, ny, ns, return_rays=True, return_camera=True, **kw)
    whole = ds.render(nx, ny, 4, 6, SEED)
    try:
        ds.render_progressive(nx, ny, 0, 2, 6, SEED)
        assert ctx.progressive_samples() == 2
        stream = torch.cuda.Stream(_dev())
        got = _device_call(ds, nx, ny, 0, ns, want_camera=True, stream=stream.cuda_stream, **kw)
        assert ctx.progressive_samples() == 2
        plin, pq, perr, pcnt = ds.render_progressive(nx, ny, 2, 2, 6, SEED)
    finally:
        ctx.progressive_release()
    assert np.array_equal(bits(plin), bits(whole[0])) and np.array_equal(pq, whole[1]) and int(pcnt[0]) == int(whole[2][0])
    for key, want in zip(("lin", "q", "se", "cnt", "rays", "cam"), host):
        assert np.array_equal(got[key].reshape(-1), np.asarray(want).reshape(-1).astype(got[key].dtype)), key
    assert (got["lin"] != -7.0).all() and (got["se"] != -7.0).all() and (got["rays"] != -7.0).all() and (got["cam"] != -7.0).all()
    # every optional output may be absent
    bare = torch.full((ny, nx, 3), -7.0, dtype=torch.float64, device=_dev()), torch.full((ny, nx), -7.0, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.render_lit_device(nx, ny, 0, ns, bare[0], bare[1], **kw)
    torch.cuda.synchronize(_dev())
    assert np.array_equal(bits(bare[0].cpu().numpy()), bits(host[0])) and np.array_equal(bits(bare[1].cpu().numpy()), bits(host[2]))


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_headers_order_launch_nothing(ctx, scenes):
    L = _ffi.lib()
    smoke = core.DeviceScene(ncs.media_flat(), ctx=ctx)
    ds = scenes("dcs", "sphere-lamp")
    nx, ny = 4, 2
    lin, se, cnt = np.full((ny, nx, 3), -7.0), np.full((ny, nx), -7.0), np.full(4, 9, np.uint64)
    state = np.zeros((nx * ny, _ffi.RAYS_REC))
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)
    err = lambda: L.rtmi_last_error().decode()

    def call(scene, nx=nx, ny=ny, s_first=0, s_count=1, depth=5, estimator=2, n_lights=0, prims=None, choice=0, precision=0, out=lin, st=None):
        return L.rtmi_render_lit(scene.handle, precision, nx, ny, s_first, s_count, depth, 1, estimator, n_lights, core.ptr(prims), choice, core.ptr(st),
                                 core.ptr(out), None, core.ptr(se), None, None, core.ptr(cnt))
    try:
        late = dict(precision=7, n_lights=len(many), prims=many, choice=5)  # what is reported later never hides what is reported first
        assert call(smoke, nx=0, estimator=9, out=None, **late) == -1 and "s_count" in err()
        assert call(smoke, s_first=-1, **late) == -1 and call(smoke, depth=-1, **late) == -1 and call(smoke, s_count=0, **late) == -1
        assert call(smoke, nx=1 << 16, ny=1 << 16, estimator=9, out=None, **late) == -1 and "2^31 - 64" in err()
        assert call(smoke, s_first=(1 << 31) - 1, estimator=9, out=None, **late) == -1 and "overflows" in err()
        assert call(smoke, estimator=9, out=None, **late) == -1 and "NULL" in err()
        assert call(smoke, estimator=9, **late) == -1 and "estimator" in err()
        assert call(smoke, **late) == -1 and "precision" in err()
        assert call(smoke, **dict(late, precision=1)) == -3                                   # RTMI_F32 on a mixed-kind scene, as rtmi_render_rays
        assert call(smoke, **dict(late, precision=0)) == -1 and "n_lights" in err()
        assert call(smoke, choice=5) == -1 and "light_choice" in err()
        assert call(smoke) == -3 and "ConstantMedium" in err() and call(smoke, estimator=1) == -3 and "ConstantMedium" in err()
        assert call(ds, n_lights=1, prims=np.array([0], np.int32)) == -1 and call(ds, n_lights=1, prims=np.array([10 ** 6], np.int32)) == -1
        bad_state = state.copy(); bad_state[:, 9] = 2
        assert call(ds, s_first=3, st=bad_state) == -5
        assert (lin == -7.0).all() and (se == -7.0).all() and (cnt == 9).all()                 # a failed call writes nothing: nothing was launched
        # estimator 0 looks at no light argument and traces the media scene; estimator 1 at no light choice
        assert call(smoke, estimator=0, **dict(late, precision=0)) == 0 and cnt.tolist()[1:] == [nx * ny, 0, 0] and (lin != -7.0).all()
        assert call(ds, estimator=1, choice=5) == 0 and cnt[2] > 0
        assert call(ds) == 0 and cnt[1] == nx * ny and call(ds, s_first=2, st=bad_state) == 0 and (bad_state[:, 9] == 3).all()
        with pytest.raises(core.RtmiError) as ei:
            smoke.render_lit(nx, ny, 1, estimator="nee")
        assert ei.value.code == -3
        assert smoke.render_lit(nx, ny, 2, estimator="plain")[3].tolist()[1:] == [2 * nx * ny, 0, 0]
        with pytest.raises(ValueError):
            ds.render_lit(nx, ny, 1, estimator="bdpt")
    finally:
        smoke.close()


# ---- 9. python and the command line ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", ("plain", "nee", "mis"))
def test_render_lit_does_not_depend_on_chunk(scenes, estimator):
    nx, ny, _ = lc.SMALL
    ds = scenes("dcs", "cornell")
    kw = dict(estimator=estimator, light_choice="power" if estimator == "mis" else 0, depth=6, seed=11, return_rays=True, return_camera=True)
    one = ds.render_lit(nx, ny, 5, **kw)
    for chunk in (1, 2, 5, 9):
        got = ds.render_lit(nx, ny, 5, chunk=chunk, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, one)), chunk
        assert np.array_equal(bits(got[0]), bits(one[0])) and np.array_equal(bits(got[2]), bits(one[2]))
    assert one[0].shape == (ny, nx, 3) and one[1].dtype == np.uint8 and one[4].shape == (nx * ny, 5, 3) and one[5].shape == (nx * ny, 5, 8)
    assert np.isfinite(one[0]).all() and (one[0].sum(axis=2) > 0).any()  # (at five samples and depth 6 the plain paths light few pixels of the box)


def test_cli_lit_writes_render_lits_frame(tmp_path):
    from raytrace_clj_amd import scene as scenes_module
    name = str(tmp_path / "box.npy")
    assert core.main([name, "13", "7", "3", "cornell-box-classic", "--lit", "mis:power", "--chunk", "2"]) == 0
    frame, lit = np.load(name), np.load(str(tmp_path / "box.lit.npy"))
    ds = core.DeviceScene(core.SCENES["cornell-box-classic"](scenes_module, 13, 7))
    try:
        want = ds.render_lit(13, 7, 3, estimator="mis", light_choice="power")[1]
        plain = ds.render_lit(13, 7, 3, estimator="plain")[1]
    finally:
        ds.close()
    assert np.array_equal(lit, want) and np.array_equal(frame, plain) and not np.array_equal(lit, frame)
