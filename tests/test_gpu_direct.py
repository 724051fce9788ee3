"""Direct lighting from first hits on the device (rtmi_scene_lights, rtmi_direct_irradiance*, rtmi_render_direct*).  The shadow rays the device
builds must equal the numpy restatement of include/rtmi.h's light rule (tests/direct_reference.py, camera.light_samples) bit for bit; the flags must
equal what rtmi_query_occluded_device answers for those numpy rays, uploaded, and the oracle's closest-hit flags; contributions, irradiance and
counters must equal the restatement's as exact doubles; and the whole pass must equal the numpy chain."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from raytrace_clj_amd import _ffi, camera, core
from tests import direct_cases as dcs
from tests import direct_reference as dref
from tests import occlusion_reference as oref

N_POINTS = dcs.N_POINTS
NX, NY = dcs.NX, dcs.NY
CASES = (("example-light", "f64"), ("cornell", "f64"), ("two-triangles", "f64"), ("sphere-lamp", "f64"), ("sphere-lamp", "f32"))
T_MIN, T_MAX = 0.001, 1.0 - 0.001


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


@functools.lru_cache(maxsize=None)
def _points(name):
    """(view rays, hit records on the host, the same in HBM, view rays in HBM): the scene's view rays through query_hits_device, then records that
    yield no ray scattered over them (idle lanes in the middle of waves).  Computed once; do not write into them."""
    import torch
    ctx, ds = _open(name)
    view = dcs.view_rays(_oracle(), name)
    d_view = torch.from_numpy(view).to(_dev())
    d_hits = torch.zeros((N_POINTS, _ffi.HIT_REC), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.query_hits_device(N_POINTS, d_view, d_hits)
    torch.cuda.synchronize(_dev())
    hits, touched = oref.degenerate(d_hits.cpu().numpy())
    assert (hits[:, 0] == 1).sum() > N_POINTS // 2 and not set(touched) & set(dcs.PLACED)
    hits, view = dcs.place(name, hits, view)  # (make_two_triangles: points whose shadow rays the triangles can occlude)
    hits, view = np.ascontiguousarray(hits), np.ascontiguousarray(view)
    d_hits, d_view = torch.from_numpy(hits).to(_dev()), torch.from_numpy(view).to(_dev())
    torch.cuda.synchronize(_dev())
    return view, hits, d_hits, d_view


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _table(name, lights=None):
    f = dcs.flat(name)
    return camera.light_table(f, dref.eligible(f) if lights is None else lights)


def _device_call(ds, n, n_samples, n_lights, d_hits, d_view, precision, state=None, **kw):
    """one rtmi_direct_irradiance_device call on HBM buffers -> (rays, flags, contributions, irradiance, counters, state) on the host"""
    import torch
    m = n * n_samples * n_lights
    d_rays = torch.full((m, 7), -7.0, dtype=torch.float64, device=_dev())
    d_flags = torch.full((m,), 9, dtype=torch.uint8, device=_dev())
    d_contrib = torch.full((m, 3), -7.0, dtype=torch.float64, device=_dev())
    d_E = torch.full((n, 3), -7.0, dtype=torch.float64, device=_dev())
    d_cnt = torch.full((2,), 9, dtype=torch.int64, device=_dev())
    d_state = torch.from_numpy(state).to(_dev()) if state is not None else None
    torch.cuda.synchronize(_dev())
    ds.direct_irradiance_device(n, d_hits, n_samples, d_E, view=d_view, state=d_state, out_contrib=d_contrib, out_occluded=d_flags, out_rays=d_rays,
                                out_counters=d_cnt, precision=precision, **kw)
    torch.cuda.synchronize(_dev())
    return (d_rays.cpu().numpy(), d_flags.cpu().numpy(), d_contrib.cpu().numpy(), d_E.cpu().numpy(), d_cnt.cpu().numpy().tolist(),
            d_state.cpu().numpy() if state is not None else None)


def _expected_flags(ds, rays, built, precision):
    """occluded_device on the numpy rays that were built, uploaded, range "up to the light"; the other items hold 0"""
    import torch
    flags = np.zeros(len(rays), np.uint8)
    some = np.ascontiguousarray(rays[built])
    d_some = torch.from_numpy(some).to(_dev())
    d_flags = torch.zeros(len(some), dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.occluded_device(len(some), 1, d_some, out_occluded=d_flags, t_min=T_MIN, t_max=T_MAX, precision=precision)
    torch.cuda.synchronize(_dev())
    flags[built] = d_flags.cpu().numpy()
    return flags


# ---- 1. the light source: rays, flags, contributions, irradiance, counters ----------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_generated_rays_and_answers(name, precision):
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    f = dcs.flat(name)
    table = _table(name)
    nl = len(table)
    assert ds.lights().tolist() == dref.eligible(f).tolist() and nl >= 1
    some_occluded = some_free = some_unbuilt = False
    for n_samples in (1, 5, 64, 70):   # 5 does not divide 64: groups straddle waves; 70: a group longer than a wave trip
        for first in (0, 3):
            for with_view in (True, False):
                v, dv = (view, d_view) if with_view else (None, None)
                lamb = first == 3
                what = "%s %s n_samples %d first %d view %s lambert_only %s" % (name, precision, n_samples, first, with_view, lamb)
                e_rays, e_w, built = dref.light_items(hits, table, n_samples, view=v, first=first, seed=77, time=0.25, lambert_only=lamb, mat_kind=f.mat_kind)
                rays, flags, contrib, E, cnt, _ = _device_call(ds, N_POINTS, n_samples, nl, d_hits, dv, precision, first=first, seed=77, time=0.25,
                                                                lambert_only=lamb)
                diff = (_bits(rays) != _bits(e_rays)).any(axis=1)
                assert not diff.any(), "%s: %d of %d rays differ from the restatement, first at item %d" % (what, diff.sum(), len(diff), int(np.flatnonzero(diff)[0]))
                e_flags = _expected_flags(ds, e_rays, built, precision)
                assert flags.dtype == np.uint8 and np.array_equal(flags, e_flags), "%s: %d flags differ" % (what, (flags != e_flags).sum())
                e_contrib = dref.contributions(e_w, built, e_flags, table)
                assert np.array_equal(_bits(contrib), _bits(e_contrib)), what + ": contributions"
                e_E, _ = dref.fold(e_contrib, N_POINTS, n_samples)  # (no state: the call's own samples)
                assert np.array_equal(_bits(E), _bits(e_E)), what + ": irradiance"
                assert cnt == [int(built.sum()), int(e_flags.sum())], (what, cnt)
                some_occluded |= bool(e_flags.any())
                some_free |= bool((e_flags[built] == 0).any())
                some_unbuilt |= bool((~built[np.repeat(oref.yields_a_ray(hits), n_samples * nl)]).any())
    # (tests/test_direct_host.py::test_points_exercise_the_rule checks the same of these points with the oracle alone)
    assert some_occluded and some_free and some_unbuilt, "%s: occluded %s free %s unbuilt %s" % (name, some_occluded, some_free, some_unbuilt)


@pytest.mark.parametrize("name", sorted({n for n, p in CASES}))
def test_flags_equal_the_oracles(name):
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    table = _table(name)
    e_rays, e_w, built = dref.light_items(hits, table, 5, view=view, seed=77)
    _, flags, _, _, _, _ = _device_call(ds, N_POINTS, 5, len(table), d_hits, d_view, "f64", seed=77)
    orc = _oracle().probe_hit(dcs.flat(name), np.ascontiguousarray(e_rays[built]), tmin=T_MIN, tmax=T_MAX)
    assert np.array_equal(flags[built], orc[:, 0].astype(np.uint8)), name
    assert not flags[~built].any()


# ---- 2. splits, host forms, a subset of the lights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("example-light", "cornell"))
def test_splits_host_forms_and_subsets(name):
    ctx, ds = _open(name)
    view, hits, d_hits, d_view = _points(name)
    table = _table(name)
    nl = len(table)
    state = np.zeros((N_POINTS, _ffi.DIRECT_REC))
    E7, cnt7, c7, f7, r7 = ds.direct_irradiance(hits, 7, view=view, seed=9, state=state, return_items=True)
    assert (E7 != 0).any() and (state[:, 3] == 7).all()
    for split in ((3, 4), (1, 5, 1)):
        st, first, total = np.zeros((N_POINTS, _ffi.DIRECT_REC)), 0, np.zeros(2, np.uint64)
        parts = []
        for n in split:
            E, cnt, c, fl_, r = ds.direct_irradiance(hits, n, view=view, first=first, seed=9, state=st, return_items=True)
            parts.append(r.reshape(N_POINTS, n, nl, 7))
            total += cnt
            first += n
        assert np.array_equal(_bits(E), _bits(E7)) and np.array_equal(_bits(st), _bits(state)), split
        assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(r7.reshape(N_POINTS, 7, nl, 7))) and total.tolist() == cnt7.tolist()
    with pytest.raises(_ffi.RtmiError) as e:  # a state that holds other samples than `first`
        ds.direct_irradiance(hits, 2, view=view, first=5, seed=9, state=state.copy())
    assert e.value.code == -5
    # the device form with a state, split the same way
    d1 = _device_call(ds, N_POINTS, 3, nl, d_hits, d_view, "f64", state=np.zeros((N_POINTS, _ffi.DIRECT_REC)), first=0, seed=9)
    d2 = _device_call(ds, N_POINTS, 4, nl, d_hits, d_view, "f64", state=d1[5], first=3, seed=9)
    assert np.array_equal(_bits(d2[3]), _bits(E7)) and np.array_equal(_bits(d2[5]), _bits(state))
    # the host form runs the device form's launches; the workspace in place of out_contrib, in passes of whole points
    rays, flags, contrib, E, cnt, _ = _device_call(ds, N_POINTS, 7, nl, d_hits, d_view, "f64", seed=9)
    assert np.array_equal(_bits(rays), _bits(r7)) and np.array_equal(flags, f7) and np.array_equal(_bits(contrib), _bits(c7))
    assert np.array_equal(_bits(E), _bits(E7)) and cnt == [int(x) for x in cnt7]
    plain, cnt_plain = ds.direct_irradiance(hits, 7, view=view, seed=9)
    assert np.array_equal(_bits(plain), _bits(E7)) and cnt_plain.tolist() == cnt7.tolist()
    small = core.Context(0)
    try:
        small.set_option("workspace_bytes", 1 << 20)  # 24 B x 7 x nl per point: several passes of whole points
        ds2 = core.DeviceScene(dcs.flat(name), ctx=small)
        passes, cnt_passes = ds2.direct_irradiance(hits, 7 * 16, view=view, seed=9)
        whole, cnt_whole = ds.direct_irradiance(hits, 7 * 16, view=view, seed=9)
        assert N_POINTS * 7 * 16 * nl * 24 > 2 * (1 << 20)
        assert np.array_equal(_bits(passes), _bits(whole)) and cnt_passes.tolist() == cnt_whole.tolist()
        ds2.close()
    finally:
        small.close()
    # a subset (and another order) of the lights equals the restatement run with that subset
    every = ds.lights().tolist()
    for subset in ([every[-1]], every[::-1]):
        sub = camera.light_table(dcs.flat(name), subset)
        e_rays, e_w, built = dref.light_items(hits, sub, 3, view=view, seed=9)
        E, cnt, c, fl_, r = ds.direct_irradiance(hits, 3, view=view, lights=subset, seed=9, return_items=True)
        assert np.array_equal(_bits(r), _bits(e_rays))
        e_c = dref.contributions(e_w, built, fl_, sub)
        assert np.array_equal(_bits(c), _bits(e_c)) and np.array_equal(_bits(E), _bits(dref.fold(e_c, N_POINTS, 3)[0]))


# ---- 3. the whole pass ------------------------------------------------------------------------------------------------------------------------
def _texture_at(ds, f, hits):
    """the material's texture at every record's (u, v, p) through rtmi_probe_texture; zeros for misses and for materials without a texture"""
    out = np.zeros((len(hits), 3))
    hit = hits[:, 0] != 0.0
    tex = np.where(hit, np.asarray(f.mat_tex)[np.where(hit, hits[:, 11], 0).astype(np.int64)], -1)
    for t in np.unique(tex[tex >= 0]):
        sel = tex == t
        out[sel] = ds.probe_texture(int(t), np.ascontiguousarray(np.concatenate([hits[sel, 9:11], hits[sel, 3:6]], axis=1)))
    return out


def _direct_chain(ds, f, nx, ny, n_samples, seed, first=0, state=None):
    """pixel_centre_rays -> query_hits -> direct_reference -> occluded -> fold -> resolve, on the host"""
    primary = ds.pixel_centre_rays(nx, ny)
    hits = ds.query_hits(primary)
    table = camera.light_table(f, dref.eligible(f))
    rays, w, built = dref.light_items(hits, table, n_samples, view=primary, first=first, seed=seed, lambert_only=True, mat_kind=f.mat_kind)
    flags = np.zeros(len(rays), np.uint8)
    flags[built] = ds.occluded(np.ascontiguousarray(rays[built]), t_min=T_MIN, t_max=T_MAX)[0]
    E, state = dref.fold(dref.contributions(w, built, flags, table), nx * ny, n_samples, first=first, state=state)
    return dref.resolve(hits, E, f.mat_kind, _texture_at(ds, f, hits)), hits, [int(built.sum()), int(flags.sum())], state


def _render_direct_device(ds, nx, ny, n_samples, **kw):
    import torch
    n = nx * ny
    lin = torch.full((n, 3), -1.0, dtype=torch.float64, device=_dev())
    q = torch.full((n, 3), 9, dtype=torch.uint8, device=_dev())
    hits = torch.full((n, _ffi.HIT_REC), -1.0, dtype=torch.float64, device=_dev())
    cnt = torch.full((2,), 9, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.render_direct_device(nx, ny, n_samples, lin, out_rgb8=q, out_hits=hits, out_counters=cnt, **kw)
    torch.cuda.synchronize(_dev())
    return lin.cpu().numpy(), q.cpu().numpy(), hits.cpu().numpy(), cnt.cpu().numpy().tolist()


@pytest.mark.parametrize("name", dcs.SCENES)
def test_whole_pass(name):
    ctx, ds = _open(name)
    f = dcs.flat(name)
    lin, q, hits, cnt = _render_direct_device(ds, NX, NY, 6, seed=31)
    e_lin, e_hits, e_cnt, e_state = _direct_chain(ds, f, NX, NY, 6, 31)
    assert np.array_equal(_bits(hits), _bits(e_hits)), "%s: %d records differ" % (name, (_bits(hits) != _bits(e_hits)).any(axis=1).sum())
    assert cnt == e_cnt and cnt[0] > 0
    assert np.array_equal(_bits(lin), _bits(e_lin)), "%s: %d pixels differ" % (name, (_bits(lin) != _bits(e_lin)).any(axis=1).sum())
    kind = np.where(hits[:, 0] != 0, np.asarray(f.mat_kind)[np.where(hits[:, 0] != 0, hits[:, 11], 0).astype(np.int64)], -1)
    dark = (kind != 0) & (kind != 3)  # misses, metal, glass
    assert not lin[dark].any()
    if name == "sphere-lamp":
        assert (kind == -1).any() and (kind == 1).any()
    emit = kind == 3
    assert emit.any() and (kind == 0).any() and (lin[kind == 0] > 0).any()
    le = np.asarray(f.tex_param, np.float64).reshape(-1, 12)[np.asarray(f.mat_tex)[hits[emit, 11].astype(np.int64)], 0:3]
    assert np.array_equal(lin[emit], le)
    assert np.array_equal(q, np.array([_oracle().quantise(p) for p in lin]))
    # the host form, with a state split over calls, and the workspace in place of out_hits
    h_lin, h_q, h_cnt, h_hits = ds.render_direct(NX, NY, 6, seed=31, return_hits=True)
    assert np.array_equal(_bits(h_lin.reshape(-1, 3)), _bits(lin)) and np.array_equal(h_q.reshape(-1, 3), q) and h_cnt.tolist() == cnt
    assert np.array_equal(_bits(h_hits), _bits(hits))
    st = np.zeros((NX * NY, _ffi.DIRECT_REC))
    ds.render_direct(NX, NY, 2, seed=31, state=st)
    s_lin, s_q, s_cnt = ds.render_direct(NX, NY, 4, first=2, seed=31, state=st)
    assert np.array_equal(_bits(s_lin.reshape(-1, 3)), _bits(lin)) and np.array_equal(s_q.reshape(-1, 3), q) and np.array_equal(_bits(st), _bits(e_state))


def test_whole_pass_f32_and_a_scene_without_lights():
    ctx, ds = _open("sphere-lamp")
    lin64 = ds.render_direct(NX, NY, 6, seed=31)[0]
    lin32, q32, cnt32 = ds.render_direct(NX, NY, 6, seed=31, precision="f32")
    # FP32 traces the same FP64 rays: only pixels on a silhouette or a shadow's edge may take another hit or flag
    close = np.isclose(lin32, lin64, rtol=1e-4, atol=1e-6).all(axis=2)
    assert lin32.shape == (NY, NX, 3) and (lin32 > 0).any() and close.mean() > 0.95, close.mean()
    import raytrace_clj_amd as r
    c2 = core.Context(0)
    cover = core.DeviceScene(r.scene.make_random_scene(NX, NY, 11, True), ctx=c2)  # its only emitter is a gradient dome: no light to sample
    try:
        assert len(cover.lights()) == 0
        lin, q, cnt = cover.render_direct(NX, NY, 4)
        hits = cover.query_hits(cover.pixel_centre_rays(NX, NY))
        kind = np.where(hits[:, 0] != 0, np.asarray(cover.flat.mat_kind)[hits[:, 11].astype(np.int64)], -1)
        assert cnt.tolist() == [0, 0] and not lin.reshape(-1, 3)[kind != 3].any()
        sky = _texture_at(cover, cover.flat, hits)
        assert (kind == 3).any() and np.array_equal(_bits(lin.reshape(-1, 3)[kind == 3]), _bits(sky[kind == 3]))  # the dome still shows its emission
        E, cnt = cover.direct_irradiance(hits, 4)
        assert not E.any() and cnt.tolist() == [0, 0]
    finally:
        cover.close()
        c2.close()


# ---- 4. arguments -------------------------------------------------------------------------------------------------------------------------------
def _idle(ctx):
    import ctypes
    idle = ctypes.c_int32(-1)
    _ffi.check(_ffi.lib().rtmi_stream_idle(ctx.handle, ctypes.byref(idle)))
    return idle.value


def test_argument_errors_launch_nothing():
    ctx, ds = _open("cornell")
    view, hits, d_hits, d_view = _points("cornell")
    import torch
    d_E = torch.zeros((N_POINTS, 3), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize(_dev())
    assert _idle(ctx) == 1
    lamp = int(ds.lights()[0])
    calls = (
        (lambda: ds.direct_irradiance(hits, 0), -1),                                             # n_samples = 0
        (lambda: ds.direct_irradiance(hits, 4, first=-1), -1),                                   # first < 0
        (lambda: ds.direct_irradiance(hits, 4, lights=[0]), -1),                                 # a wall is not a light
        (lambda: ds.direct_irradiance(hits, 4, lights=[lamp, 12]), -1),                          # nor is an instanced block's face
        (lambda: ds.direct_irradiance(hits, 4, lights=[lamp, 9999]), -1),                        # nor a primitive that does not exist
        (lambda: ds.direct_irradiance(hits, 4, lights=[-1]), -1),
        (lambda: ds.direct_irradiance(hits, 1, lights=[lamp] * 33), -1),                         # 33 lights
        (lambda: ds.direct_irradiance_device(N_POINTS, None, 4, d_E), -1),                       # NULL hits
        (lambda: ds.direct_irradiance_device(N_POINTS, d_hits, 4, None), -1),                    # NULL out_irradiance
        (lambda: ds.direct_irradiance_device(2 ** 30, d_hits, 4, d_E), -1),                      # a product beyond 2^31 - 64
        (lambda: ds.direct_irradiance_device(4, d_hits, 2 ** 30, d_E, lights=[lamp] * 4), -1),
        (lambda: ds.render_direct_device(NX, NY, 0, d_E), -1),
        (lambda: ds.render_direct_device(NX, NY, 4, None), -1),                                  # NULL out_linear
        (lambda: ds.render_direct_device(2 ** 15, 2 ** 15, 4, d_E), -1),
        (lambda: ds.direct_irradiance(hits, 4, precision="f32"), -3),                            # RTMI_F32 on a mixed-kind scene
        (lambda: ds.render_direct(NX, NY, 4, precision="f32"), -3),
    )
    for call, code in calls:
        with pytest.raises(_ffi.RtmiError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert _idle(ctx) == 1
    assert "FP64 only" in str(e.value)
    E, cnt = ds.direct_irradiance(hits, 1, lights=[lamp] * 32)  # 32 lights is the most: the lamp 32 times over is 32 times one lamp's estimate ...
    assert (E > 0).any() and cnt[0] > 0                           # ... from other samples (each copy has its own streams)


def test_nothing_to_do_is_ok():
    ctx, ds = _open("example-light")
    E, cnt = ds.direct_irradiance(np.zeros((0, _ffi.HIT_REC)), 4)
    assert E.shape == (0, 3) and list(cnt) == [0, 0]
    ds.direct_irradiance_device(0, None, 4, None)
    assert ds.render_direct(0, NY, 4)[0].shape == (NY, 0, 3) and ds.render_direct(NX, 0, 4)[0].shape == (0, NX, 3)
    ds.render_direct_device(0, 0, 4, None)
    view, hits, d_hits, d_view = _points("example-light")
    E, cnt, c, f, r = ds.direct_irradiance(hits, 4, lights=[], return_items=True)  # zero lights: zeros, nothing launched
    assert E.shape == (N_POINTS, 3) and not E.any() and list(cnt) == [0, 0] and len(c) == 0


def test_missing_texture_tables_are_an_error_not_a_launch():
    """the resolve samples textures: a Perlin texture without its tables, or an ImageMap without its images, is refused as rtmi_render refuses it"""
    import copy
    import raytrace_clj_amd as r
    from raytrace_clj_amd import flatten as fl
    import torch
    perlin = copy.copy(fl.flatten(r.scene.make_two_perlin_spheres(NX, NY)))
    assert perlin.perlin_vectors is not None
    perlin.perlin_vectors = None  # DeviceScene then makes no rtmi_scene_set_perlin call
    image = copy.copy(fl.flatten(r.scene.make_textured_sphere(NX, NY)))
    assert len(image.images) > 0
    image.images = []             # ... and no rtmi_scene_set_images call
    d_lin = torch.zeros((NX * NY, 3), dtype=torch.float64, device=_dev())
    torch.cuda.synchronize(_dev())
    for f, words in ((perlin, "rtmi_scene_set_perlin"), (image, "rtmi_scene_set_images")):
        ctx = core.Context(0)
        ds = core.DeviceScene(f, ctx=ctx)
        try:
            for call in (lambda: ds.render_direct(NX, NY, 2), lambda: ds.render_direct_device(NX, NY, 2, d_lin),
                         lambda: ds.render(NX, NY, 1)):  # (the last: the refusal this one mirrors)
                with pytest.raises(_ffi.RtmiError) as e:
                    call()
                assert e.value.code == -5 and words in str(e.value), str(e.value)
                assert _idle(ctx) == 1
        finally:
            ds.close()
            ctx.close()


def test_a_state_continues_on_a_scene_without_lights():
    import raytrace_clj_amd as r
    import torch
    ctx = core.Context(0)
    cover = core.DeviceScene(r.scene.make_random_scene(NX, NY, 11, True), ctx=ctx)  # its only emitter is a gradient dome
    try:
        n = NX * NY
        one = cover.render_direct(NX, NY, 6)
        st = np.full((n, _ffi.DIRECT_REC), -7.0)
        a = cover.render_direct(NX, NY, 2, state=st)
        assert np.array_equal(st, np.tile([0.0, 0.0, 0.0, 2.0], (n, 1)))
        b = cover.render_direct(NX, NY, 4, first=2, state=st)
        assert np.array_equal(st, np.tile([0.0, 0.0, 0.0, 6.0], (n, 1)))
        for got in (a, b):
            assert np.array_equal(_bits(got[0]), _bits(one[0])) and np.array_equal(got[1], one[1]) and got[2].tolist() == [0, 0]
        # the device form writes the same records
        d_st = torch.full((n, _ffi.DIRECT_REC), -7.0, dtype=torch.float64, device=_dev())
        d_lin = torch.zeros((n, 3), dtype=torch.float64, device=_dev())
        torch.cuda.synchronize(_dev())
        cover.render_direct_device(NX, NY, 2, d_lin, state=d_st)
        cover.render_direct_device(NX, NY, 4, d_lin, first=2, state=d_st)
        torch.cuda.synchronize(_dev())
        assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(_bits(d_lin.cpu().numpy()), _bits(one[0].reshape(-1, 3)))
    finally:
        cover.close()
        ctx.close()
    # an empty list of lights on a scene that has some: the sums carry over, the samples count, E = sum * (1 / samples)
    ctx, ds = _open("example-light")
    view, hits, d_hits, d_view = _points("example-light")
    st = np.zeros((N_POINTS, _ffi.DIRECT_REC))
    E3, _ = ds.direct_irradiance(hits, 3, view=view, seed=9, state=st)
    sums = st[:, 0:3].copy()
    assert sums.any() and (st[:, 3] == 3).all()
    E5, cnt = ds.direct_irradiance(hits, 2, view=view, lights=[], first=3, seed=9, state=st)
    e_E, e_st = sums * (1.0 / 5.0), np.concatenate([sums, np.full((N_POINTS, 1), 5.0)], axis=1)  # the fold over no items
    assert np.array_equal(_bits(st), _bits(e_st)) and np.array_equal(_bits(E5), _bits(e_E)) and cnt.tolist() == [0, 0] and (st[:, 3] == 5).all()
    d_st = torch.from_numpy(np.concatenate([sums, np.full((N_POINTS, 1), 3.0)], axis=1)).to(_dev())
    d_E = torch.full((N_POINTS, 3), -7.0, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize(_dev())
    ds.direct_irradiance_device(N_POINTS, d_hits, 2, d_E, view=d_view, lights=[], first=3, seed=9, state=d_st)
    torch.cuda.synchronize(_dev())
    assert np.array_equal(_bits(d_st.cpu().numpy()), _bits(st)) and np.array_equal(_bits(d_E.cpu().numpy()), _bits(E5))
    fresh = np.full((N_POINTS, _ffi.DIRECT_REC), -7.0)
    E0, _ = ds.direct_irradiance(hits, 2, view=view, lights=[], state=fresh)
    assert not E0.any() and np.array_equal(fresh, np.tile([0.0, 0.0, 0.0, 2.0], (N_POINTS, 1)))


def test_cli_direct_writes_the_lit_view(tmp_path, capsys):
    import raytrace_clj_amd as r
    name = str(tmp_path / "view.npy")
    assert core.main([name, "16", "8", "1", "example-light", "--direct", "3"]) == 0
    capsys.readouterr()
    lit = np.load(str(tmp_path / "view.direct.npy"))
    ds = core.DeviceScene(r.scene.make_example_light(16, 8))
    try:
        exp = ds.render_direct(16, 8, 3)[1]
    finally:
        ds.close()
    assert exp.any() and lit.dtype == np.uint8 and np.array_equal(lit, exp)


# ---- 5. edits -------------------------------------------------------------------------------------------------------------------------------------
def test_lights_follow_material_edits():
    import copy
    f7 = dcs.flat("cornell")
    lamp_tex = int(f7.mat_tex[int(f7.prim_mat[int(dref.eligible(f7)[0])])])
    f3 = copy.copy(f7)
    f3.tex_param = np.array(f7.tex_param, np.float64).reshape(-1, 12).copy()
    assert f3.tex_param[lamp_tex, 0:3].tolist() == [7.0, 7.0, 7.0]
    f3.tex_param[lamp_tex, 0:3] = 3.0
    ctx = core.Context(0)
    edited, fresh = core.DeviceScene(f7, ctx=ctx), core.DeviceScene(f3, ctx=ctx)
    try:
        before = edited.render_direct(NX, NY, 4, seed=5)
        assert edited.set_materials(f3) is False
        after, new = edited.render_direct(NX, NY, 4, seed=5), fresh.render_direct(NX, NY, 4, seed=5)
        assert np.array_equal(_bits(after[0]), _bits(new[0])) and np.array_equal(after[1], new[1]) and after[2].tolist() == new[2].tolist()
        assert not np.array_equal(before[0], after[0]) and edited.lights().tolist() == fresh.lights().tolist()
        lit = before[0] > 0
        assert np.allclose(after[0][lit], before[0][lit] * (3.0 / 7.0), rtol=1e-12, atol=0)
        # an edit that turns the lamp into a gradient emitter leaves the scene without lights
        f0 = copy.copy(f3)
        f0.tex_kind = np.array(f3.tex_kind, np.int32)
        f0.tex_kind[lamp_tex] = 1
        edited.set_materials(f0)
        assert len(edited.lights()) == 0 and edited.render_direct(NX, NY, 4, seed=5)[2].tolist() == [0, 0]
    finally:
        edited.close()
        fresh.close()
        ctx.close()
