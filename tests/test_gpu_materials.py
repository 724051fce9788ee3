"""The materials and textures of a live scene on the device (rtmi_scene_set_materials, rtmi_scene_set_materials_stream).  Every comparison is
np.array_equal of linear frame, 8-bit frame and ray counters between the LIVE scene after set_materials and a DeviceScene created FRESH from
the edited FlatScene.  All frames are 36x20 (partial 8x8 tiles on both edges), 4 samples, depth 50.  The edits are made on the flat arrays: a
material or texture is found by its kind, not by its place, so the cases do not depend on the flattener's interning order."""
import copy
import ctypes as C

import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi, core, dist, perlin
from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import flatten as fl

pytestmark = pytest.mark.gpu

NX, NY, NS = 36, 20, 4
ASPECT = float(np.float32(NX)) / float(np.float32(NY))
RTMI_E_ARG, RTMI_E_UNSUPPORTED, RTMI_E_STATE = -1, -3, -5
TABLES = ("mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child", "prim_mat")


def _edit(flat, change=None):
    """a copy of `flat` whose material arrays are its own, changed by change(f)"""
    f = copy.copy(flat)
    for name in TABLES:
        setattr(f, name, np.array(getattr(flat, name)))
    if change is not None:
        change(f)
    return f


def _with_camera(flat, camera):
    f = copy.copy(flat)
    f.cam_kind, f.cam = fl.flatten_camera(camera)
    return f


def _fresh(flat, ctx, render):
    """render(ds) of a scene created fresh from `flat`"""
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        return render(ds)
    finally:
        ds.close()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _frame(precision="f64"):
    return lambda ds: ds.render(NX, NY, NS, precision=precision)


def _bytes(ds):
    n = C.c_int64()
    core.check(_ffi.lib().rtmi_scene_device_bytes(ds.handle, C.byref(n)))
    return n.value


def _first(mask):
    idx = np.flatnonzero(mask)
    assert len(idx), "the scene holds no such record"
    return int(idx[0])


def _used(f, kind):
    """first material of `kind` that a primitive uses"""
    return _first((f.mat_kind == kind) & np.isin(np.arange(len(f.mat_kind)), f.prim_mat))


def _raw_args(f, prim_mat=True):
    a = [np.ascontiguousarray(x, dt) for x, dt in ((f.mat_kind, np.int32), (f.mat_tex, np.int32), (f.mat_param, np.float64), (f.tex_kind, np.int32),
                                                   (f.tex_param, np.float64), (f.tex_child, np.int32), (f.prim_mat, np.int32))]
    p = _ffi.ptr
    return a, (len(a[0]), p(a[0]), p(a[1]), p(a[2]), len(a[3]), p(a[3]), p(a[4]), p(a[5]), p(a[6]) if prim_mat else None)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


# ---- 1. the sphere kernels --------------------------------------------------------------------------------------------------------------------
def _sphere_edit(f):
    """a Constant colour, a metal's fuzz, a dielectric's index, a Lambertian into a Metal, the checker's scale -- each where the scene has one;
    -> the names of the edits made"""
    done = ["scale", "colour"]
    used = lambda kind: [int(m) for m in np.flatnonzero(f.mat_kind == kind) if m in f.prim_mat]
    metals, glass, lamb = used(fl.MAT_METAL), used(fl.MAT_DIELECTRIC), used(fl.MAT_LAMBERTIAN)
    checker = _first(f.tex_kind == fl.TEX_CHECKER)
    f.tex_param[checker, 0] = 3.0
    f.tex_param[f.tex_child[checker, 0], 0:3] = (0.8, 0.1, 0.3)  # a Constant inside the checker (the record's CHECKER2 colours)
    plain = [m for m in lamb if f.tex_kind[f.mat_tex[m]] == fl.TEX_CONSTANT]
    if plain:
        f.tex_param[f.mat_tex[plain[0]], 0:3] = (0.1, 0.6, 0.9)  # a Constant that a material holds directly
    turned = plain[1] if len(plain) > 1 else lamb[0]
    f.mat_kind[turned], f.mat_param[turned] = fl.MAT_METAL, 0.3
    done.append("lambertian->metal")
    if glass:
        f.mat_param[glass[0]] = 2.4
        done.append("index")
    if metals:
        f.mat_param[metals[0]] = 0.45
        done.append("fuzz")
    return done


SPHERE_SCENES = {
    "cover-bvh": lambda: r.scene.make_random_scene(NX, NY, 3, False),
    "cover-list": lambda: r.scene.make_random_scene(NX, NY, 3, False, bvh=False),
    "two-spheres": lambda: r.scene.make_two_spheres(NX, NY),
}


@pytest.mark.parametrize("name", sorted(SPHERE_SCENES))
def test_sphere_scenes_follow_an_edit(ctx, name):
    flat = fl.flatten(SPHERE_SCENES[name]())
    done = []
    edited = _edit(flat, lambda f: done.extend(_sphere_edit(f)))
    assert {"scale", "colour", "lambertian->metal"} <= set(done)
    if name.startswith("cover"):
        assert set(done) == {"scale", "colour", "lambertian->metal", "index", "fuzz"}
    assert any(not np.array_equal(getattr(flat, t), getattr(edited, t)) for t in TABLES)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size, info = _bytes(live), live.tree_info()
        assert live.set_materials(edited) is False
        assert _bytes(live) == size and live.tree_info() == info
        assert live.flat is not flat and np.array_equal(live.flat.mat_param, edited.mat_param) and np.array_equal(flat.mat_kind, fl.flatten(SPHERE_SCENES[name]()).mat_kind)
        for precision in ("f64", "f32"):
            got, want = _frame(precision)(live), _fresh(edited, ctx, _frame(precision))
            assert _same(got, want), (name, precision, float(np.abs(got[0] - want[0]).max()))
            assert got[2][1] == NX * NY
        assert not _same(_frame()(live)[:2], _fresh(flat, ctx, _frame())[:2])  # the edit is visible
        # Shader.scatter of an edited material, as the probe sees it
        rng = np.random.default_rng(5)
        n = 96
        nrm = rng.normal(0, 1, (n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        p = rng.normal(0, 3, (n, 3))
        hits = np.concatenate([p, nrm, rng.random((n, 2))], axis=1)
        rays = np.concatenate([p + nrm, -nrm + 0.2 * rng.normal(0, 1, (n, 3)), rng.random((n, 1))], axis=1)
        keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
        for m in np.flatnonzero((flat.mat_kind != edited.mat_kind) | (flat.mat_param != edited.mat_param)):
            for precision in ("f64", "f32"):
                probe = lambda ds: (ds.probe_scatter(int(m), rays, hits, keys, precision),)
                assert _same(probe(live), _fresh(edited, ctx, probe)), (name, int(m), precision)
    finally:
        live.close()


def test_the_traversal_counters_equal_a_fresh_scene_after_an_edit_in_place(ctx):
    """the tree is untouched and a fresh scene builds the same one: node visits and leaf tests agree too"""
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    edited = _edit(flat, _sphere_edit)

    def counted(ds):
        ctx.set_option("count_traversal", 1)
        try:
            ds.render(NX, NY, NS)
            return ctx.last_traversal_counters()
        finally:
            ctx.set_option("count_traversal", 0)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        assert live.set_materials(edited) is False
        got, want = counted(live), _fresh(edited, ctx, counted)
        assert tuple(got) == tuple(want) and got[0] > 0
    finally:
        live.close()


# ---- 2. the EXT kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", ["0", "24"], ids=["tree", "small-scan"])
def test_cornell_box_follows_an_edit(ctx, monkeypatch, below):
    monkeypatch.setenv("RTMI_FLAT_BELOW", below)  # read per render: 24 answers the request for the tree with the small scan
    flat = fl.flatten(r.scene.make_cornell_box(NX, NY))

    def change(f):
        light = _used(f, fl.MAT_DIFFUSE_LIGHT)
        f.tex_param[f.mat_tex[light], 0:3] = (15.0, 12.0, 9.0)
        walls = [m for m in np.flatnonzero(f.mat_kind == fl.MAT_LAMBERTIAN)][:2]
        assert len(walls) == 2
        f.tex_param[f.mat_tex[walls[0]], 0:3] = (0.1, 0.2, 0.7)
        f.tex_param[f.mat_tex[walls[1]], 0:3] = (0.6, 0.6, 0.2)
    edited = _edit(flat, change)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size, info = _bytes(live), live.tree_info()
        assert live.set_materials(edited) is False and _bytes(live) == size and live.tree_info() == info
        got = _frame()(live)
        assert ctx.last_accel() == ("flat" if below == "24" else "bvh")
        assert _same(got, _fresh(edited, ctx, _frame()))
        assert not _same(got[:2], _fresh(flat, ctx, _frame())[:2])
    finally:
        live.close()


# ---- 3. the NEEDS_* bits of the primitives ----------------------------------------------------------------------------------------------------
def test_textured_sphere_uv_bits_follow_the_texture(ctx):
    """the UVSphere's material points at FlipV(ImageMap) (reads u and v), then at a Constant (reads neither: the device skips the sphere's uv),
    then at the image again: both edits in place, each equal to fresh"""
    flat = fl.flatten(r.scene.make_textured_sphere(NX, NY, r.scene.synthetic_earth(64, 32)))
    globe = int(flat.prim_mat[_first(flat.prim_kind == fl.PRIM_UVSPHERE)])
    assert flat.tex_kind[flat.mat_tex[globe]] == fl.TEX_FLIP_V
    plain = _edit(flat, lambda f: f.mat_tex.__setitem__(globe, _first(f.tex_kind == fl.TEX_CONSTANT)))
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size = _bytes(live)
        first = _frame()(live)
        assert live.set_materials(plain) is False and _bytes(live) == size
        got = _frame()(live)
        assert _same(got, _fresh(plain, ctx, _frame())) and not _same(got[:2], first[:2])
        assert live.set_materials(flat) is False and _bytes(live) == size
        assert _same(_frame()(live), first) and _same(first, _fresh(flat, ctx, _frame()))
    finally:
        live.close()


def test_rectangle_uv_bits_follow_the_texture(ctx):
    """Cornell box: one wall's Constant becomes a UVGradient whose corners vary (its rectangles compute uv now), another wall's a checker over
    that gradient and a Constant (uv through a child); then back: the bits are cleared again"""
    flat = fl.flatten(r.scene.make_cornell_box(NX, NY))
    walls = [int(m) for m in np.flatnonzero(flat.mat_kind == fl.MAT_LAMBERTIAN)]
    assert len(walls) >= 3 and (flat.tex_kind == fl.TEX_CONSTANT).all()
    ta, tb, tc = (int(flat.mat_tex[m]) for m in walls[:3])

    def change(f):
        f.tex_kind[ta] = fl.TEX_UVGRADIENT
        f.tex_param[ta] = (0.9, 0.1, 0.1, 0.1, 0.9, 0.1, 0.1, 0.1, 0.9, 0.8, 0.8, 0.1)
        f.tex_kind[tb] = fl.TEX_CHECKER
        f.tex_param[tb, 0] = 0.02
        f.tex_child[tb] = (ta, tc)
    edited = _edit(flat, change)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size = _bytes(live)
        first = _frame()(live)
        assert live.set_materials(edited) is False and _bytes(live) == size
        got = _frame()(live)
        assert _same(got, _fresh(edited, ctx, _frame())) and not _same(got[:2], first[:2])
        assert live.set_materials(flat, stream=0) is False  # the way back travels as rows on the stream
        assert _same(_frame()(live), first)
    finally:
        live.close()


def test_triangle_uv_bits_follow_the_texture(ctx):
    flat = fl.flatten(r.scene.make_two_triangles(NX, NY))
    tri = int(flat.prim_mat[_first(flat.prim_kind == fl.PRIM_TRIANGLE)])
    t = int(flat.mat_tex[tri])

    def change(f):
        f.tex_kind[t] = fl.TEX_UVGRADIENT
        f.tex_param[t] = (0.9, 0.1, 0.1, 0.1, 0.9, 0.1, 0.1, 0.1, 0.9, 0.8, 0.8, 0.1)
    edited = _edit(flat, change)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        assert live.set_materials(edited) is False
        assert _same(_frame()(live), _fresh(edited, ctx, _frame()))
    finally:
        live.close()


# ---- 4. the assignment ------------------------------------------------------------------------------------------------------------------------
def test_prim_mat_is_swapped_and_null_keeps_it(ctx):
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    a = _first(flat.mat_kind[flat.prim_mat] == fl.MAT_METAL)
    b = _first(flat.mat_kind[flat.prim_mat] == fl.MAT_DIELECTRIC)

    def swap(f):
        f.prim_mat[a], f.prim_mat[b] = flat.prim_mat[b], flat.prim_mat[a]
    swapped = _edit(flat, swap)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        assert live.set_materials(swapped) is False
        got = _frame()(live)
        assert _same(got, _fresh(swapped, ctx, _frame())) and not _same(got[:2], _fresh(flat, ctx, _frame())[:2])
        # prim_mat = NULL: other tables, the swapped assignment stays
        recoloured = _edit(swapped, lambda f: f.tex_param.__setitem__((_first(f.tex_kind == fl.TEX_CHECKER), 0), 2.0))
        keep, args = _raw_args(recoloured, prim_mat=False)
        rebuilt = C.c_int32(-1)
        core.check(_ffi.lib().rtmi_scene_set_materials(live.handle, *args, C.byref(rebuilt)))
        assert rebuilt.value == 0
        assert _same(_frame()(live), _fresh(recoloured, ctx, _frame()))
        keep, args = _raw_args(swapped, prim_mat=False)
        core.check(_ffi.lib().rtmi_scene_set_materials_stream(live.handle, *args, None))
        assert _same(_frame()(live), got)
    finally:
        live.close()


# ---- 5. an edit that does not fit -------------------------------------------------------------------------------------------------------------
def test_an_edit_that_does_not_fit_rebuilds_or_is_refused_on_the_stream(ctx):
    flat = fl.flatten(r.scene.make_two_spheres(NX, NY))
    slot = int(flat.tex_child[_first(flat.tex_kind == fl.TEX_CHECKER), 1])
    assert flat.tex_kind[slot] == fl.TEX_CONSTANT

    def to_perlin(f):  # the slot is reused: the texture count stays, but the scene needs the EXT kernels now
        f.tex_kind[slot] = fl.TEX_PERLIN_NOISE
        f.tex_param[slot] = 0.0
        f.tex_param[slot, 0] = 4.0
    edited = _edit(flat, to_perlin)
    edited.perlin_vectors, edited.perlin_perm = perlin.make_tables(perlin.PERLIN_SEED)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        handle, before = live.handle.value, _frame()(live)
        with pytest.raises(core.RtmiError) as e:
            live.set_materials(edited, stream=0)
        assert e.value.code == RTMI_E_UNSUPPORTED and "has_ext" in str(e.value) and "rtmi_scene_set_materials" in str(e.value)
        assert live.flat is flat and _same(_frame()(live), before)
        assert live.set_materials(edited) is True and live.handle.value == handle
        with pytest.raises(core.RtmiError) as e:
            _frame()(live)
        assert e.value.code == RTMI_E_STATE  # a Perlin texture without its tables, as for a fresh scene
        vec, perm = np.ascontiguousarray(edited.perlin_vectors, np.float64), np.ascontiguousarray(edited.perlin_perm, np.int32)
        core.check(_ffi.lib().rtmi_scene_set_perlin(live.handle, _ffi.ptr(vec), _ffi.ptr(perm)))
        got = _frame()(live)
        assert _same(got, _fresh(edited, ctx, _frame())) and not _same(got[:2], before[:2])
        # ... and back: the last EXT texture leaves, the sphere kernels (and FP32) return
        assert live.set_materials(flat) is True
        assert _same(_frame()(live), before) and _same(_frame("f32")(live), _fresh(flat, ctx, _frame("f32")))
    finally:
        live.close()


def test_another_material_count_rebuilds(ctx):
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    prim = _first(flat.mat_kind[flat.prim_mat] == fl.MAT_LAMBERTIAN)

    def grow(f):  # one more material (a mirror over an existing texture), given to one primitive
        f.mat_kind = np.append(f.mat_kind, fl.MAT_METAL).astype(np.int32)
        f.mat_tex = np.append(f.mat_tex, f.mat_tex[f.prim_mat[prim]]).astype(np.int32)
        f.mat_param = np.append(f.mat_param, 0.05)
        f.prim_mat[prim] = len(f.mat_kind) - 1
    grown = _edit(flat, grow)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        with pytest.raises(core.RtmiError) as e:
            live.set_materials(grown, stream=0)
        assert e.value.code == RTMI_E_UNSUPPORTED and "materials" in str(e.value)
        assert live.set_materials(grown) is True
        assert _same(_frame()(live), _fresh(grown, ctx, _frame()))
        assert live.set_materials(_edit(grown, lambda f: f.mat_param.__setitem__(-1, 0.5))) is False  # the new count is the scene's now
    finally:
        live.close()


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------------------
def test_a_render_queued_before_the_stream_form_keeps_the_old_materials(ctx):
    import torch
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    edited = _edit(flat, _sphere_edit)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        dev = "cuda:%d" % ctx.device
        out = [torch.zeros((NY, NX, 3), dtype=torch.float64, device=dev) for _ in range(3)]
        q = [torch.zeros((NY, NX, 3), dtype=torch.uint8, device=dev) for _ in range(3)]
        cnt = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(3)]
        torch.cuda.synchronize(ctx.device)
        live.render_device(NX, NY, NS, out[0], q[0], cnt[0])      # old materials
        assert live.set_materials(edited, stream=0) is False      # no wait: the host mirror changes at once
        live.render_device(NX, NY, NS, out[1], q[1], cnt[1])      # new materials
        assert live.set_materials(edited, stream=0) is False      # nothing changes: nothing is launched
        live.render_device(NX, NY, NS, out[2], q[2], cnt[2])
        torch.cuda.synchronize(ctx.device)
        got = [(out[k].cpu().numpy(), q[k].cpu().numpy(), cnt[k].cpu().numpy().astype(np.uint64)) for k in range(3)]
        old, new = _fresh(flat, ctx, _frame()), _fresh(edited, ctx, _frame())
        assert _same(got[0], old) and _same(got[1], new) and _same(got[2], new) and not _same(old[:2], new[:2])
    finally:
        live.close()


# ---- 7. the cap of the stream form ------------------------------------------------------------------------------------------------------------
def test_the_stream_form_refuses_more_than_its_cap(ctx):
    flat = fl.flatten(r.scene.make_random_scene(NX, NY, 11, False))

    def everything(f):
        const = f.tex_kind == fl.TEX_CONSTANT
        f.tex_param[const, 0:3] = 1.0 - f.tex_param[const, 0:3] * 0.5
        f.mat_param[f.mat_kind == fl.MAT_METAL] *= 0.5
        f.mat_param[f.mat_kind == fl.MAT_DIELECTRIC] = 1.8
    edited = _edit(flat, everything)
    rows = 96 * int((flat.tex_param != edited.tex_param).any(axis=1).sum())  # 96 bytes of parameters per changed texture
    assert rows > _ffi.EDIT_STREAM_MAX_BYTES, "the texture parameters alone exceed the cap (%d bytes)" % rows
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size, info, before = _bytes(live), live.tree_info(), _frame()(live)
        with pytest.raises(core.RtmiError) as e:
            live.set_materials(edited, stream=0)
        assert e.value.code == RTMI_E_UNSUPPORTED and "RTMI_EDIT_STREAM_MAX_BYTES" in str(e.value)
        assert live.flat is flat and _same(_frame()(live), before)
        assert live.set_materials(edited) is False and _bytes(live) == size and live.tree_info() == info
        got = _frame()(live)
        assert _same(got, _fresh(edited, ctx, _frame())) and not _same(got[:2], before[:2])
        # a few records of the same scene travel on the stream
        few = _edit(edited, lambda f: f.mat_param.__setitem__(_used(f, fl.MAT_DIELECTRIC), 1.3))
        assert live.set_materials(few, stream=0) is False
        assert _same(_frame()(live), _fresh(few, ctx, _frame()))
    finally:
        live.close()


def test_a_stream_edit_of_several_launches(ctx):
    """more changed rows than one launch carries (64 rows, 704 words), fewer bytes than the cap: the batches are queued back to back"""
    flat = fl.flatten(r.scene.make_random_scene(NX, NY, 11, False))
    plain = [int(m) for m in np.flatnonzero(flat.mat_kind == fl.MAT_LAMBERTIAN) if flat.tex_kind[flat.mat_tex[m]] == fl.TEX_CONSTANT][:100]
    assert len(plain) == 100 and len(set(flat.mat_tex[plain])) == 100

    def change(f):
        f.tex_param[f.mat_tex[plain], 0:3] = 0.25 + 0.5 * f.tex_param[f.mat_tex[plain], 0:3]
    edited = _edit(flat, change)  # per material: 96 bytes of texture parameters + 96 of material record
    assert 64 < 2 * len(plain) and 192 * len(plain) <= _ffi.EDIT_STREAM_MAX_BYTES
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        before = _frame()(live)
        assert live.set_materials(edited, stream=0) is False
        got = _frame()(live)
        assert _same(got, _fresh(edited, ctx, _frame())) and not _same(got[:2], before[:2])
    finally:
        live.close()


# ---- 8. validation ----------------------------------------------------------------------------------------------------------------------------
def test_bad_edits_give_creations_errors_and_change_nothing(ctx):
    flat = fl.flatten(r.scene.make_subsurface_sphere(NX, NY))
    medium = _first((flat.prim_kind & ~fl.PRIM_BOUNDARY) == fl.PRIM_MEDIUM)
    bad = {
        "texture index": _edit(flat, lambda f: f.mat_tex.__setitem__(_used(f, fl.MAT_LAMBERTIAN), len(f.tex_kind))),
        "RTMI_MAT_ISOTROPIC": _edit(flat, lambda f: f.mat_kind.__setitem__(int(f.prim_mat[medium]), fl.MAT_LAMBERTIAN)),
        "material index": _edit(flat, lambda f: f.prim_mat.__setitem__(0, len(f.mat_kind))),
    }
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        size, before = _bytes(live), _frame()(live)
        live.render_progressive(NX, NY, 0, 2)
        for what, f in bad.items():
            with pytest.raises(core.RtmiError) as created:
                core.DeviceScene(f, ctx=ctx)
            for stream in (None, 0):
                with pytest.raises(core.RtmiError) as e:
                    live.set_materials(f, stream=stream)
                assert e.value.code == created.value.code == RTMI_E_ARG and what in str(e.value), (what, str(e.value))
        assert live.flat is flat and _bytes(live) == size
        live.render_progressive(NX, NY, 2, 2)  # not even the revision moved: the frame started before goes on
        ctx.progressive_release()
        assert _same(_frame()(live), before)
    finally:
        ctx.progressive_release()
        live.close()


# ---- 9. progressive frames --------------------------------------------------------------------------------------------------------------------
def test_progressive_frame_is_not_continued_across_an_edit(ctx):
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    edited = _edit(flat, _sphere_edit)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        for stream, f in ((None, edited), (0, flat), (None, flat)):  # the last one sets what the scene already has: the revision moves all the same
            live.render_progressive(NX, NY, 0, 2)
            live.set_materials(f, stream=stream)
            with pytest.raises(core.RtmiError) as e:
                live.render_progressive(NX, NY, 2, 2)
            assert e.value.code == RTMI_E_STATE
            with pytest.raises(core.RtmiError) as e:
                live.render_adaptive(NX, NY, 2, 2, 0.05)
            assert e.value.code == RTMI_E_STATE
            lin, q, err, cnt = live.render_progressive(NX, NY, 0, NS)
            assert _same((lin, q, cnt), _fresh(f, ctx, _frame()))
    finally:
        ctx.progressive_release()
        live.close()


# ---- 10. what replays the scene's arguments ----------------------------------------------------------------------------------------------------
def test_a_clone_made_after_an_edit_holds_it(ctx):
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    edited = _edit(flat, _sphere_edit)
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        live.set_materials(edited, stream=0)
        twin = live.clone(ctx)
        try:
            assert twin.flat is live.flat
            assert _same(_frame()(twin), _fresh(edited, ctx, _frame()))
            twin.set_materials(flat)  # the clone's copy of flat is its own: the original keeps the edit
            assert live.flat is not twin.flat and _same(_frame()(live), _fresh(edited, ctx, _frame()))
        finally:
            twin.close()
    finally:
        live.close()


def test_a_camera_rebuild_after_an_edit_keeps_it(ctx):
    """moving spheres built for the shutter [0.25, 0.5], their materials edited in place, then the scene's own camera ([0, 1]): the rebuild
    starts from the arguments the scene holds NOW"""
    sc = r.scene.make_random_scene(NX, NY, 3, True)
    flat, own = fl.flatten(sc), sc["camera"]
    narrow = cam.thin_lens_camera(lookfrom=[13.0, 2.0, 3.0], lookat=[0.0, 0.0, 0.0], vup=[0.0, 1.0, 0.0], vfov=20.0, aspect=ASPECT, aperture=0.0,
                                  focus_dist=10.0, t0=0.25, t1=0.5)
    edited = _edit(flat, _sphere_edit)
    for stream in (None, 0):
        live = core.DeviceScene(_with_camera(flat, narrow), ctx=ctx)
        try:
            assert live.set_materials(edited, stream=stream) is False
            assert _same(_frame()(live), _fresh(_with_camera(edited, narrow), ctx, _frame()))
            assert live.set_camera(own) is True
            assert _same(_frame()(live), _fresh(_with_camera(edited, own), ctx, _frame()))
        finally:
            live.close()


def test_replicas_follow_an_edit(ctx):
    flat = fl.flatten(SPHERE_SCENES["cover-bvh"]())
    edited = _edit(flat, _sphere_edit)
    md = dist.MultiDevice(flat, [0, 0])
    try:
        assert md.set_materials(edited) is False
        assert _same(md.render(NX, NY, NS), _fresh(edited, ctx, _frame()))
        # a bad edit is refused before the first replica is written
        bad = _edit(edited, lambda f: f.mat_tex.__setitem__(_used(f, fl.MAT_LAMBERTIAN), -3))
        with pytest.raises(core.RtmiError) as e:
            md.set_materials(bad)
        assert e.value.code == RTMI_E_ARG
        with pytest.raises(ValueError):
            md.set_materials(fl.flatten(r.scene.make_two_spheres(NX, NY)))
        assert _same(md.render(NX, NY, NS), _fresh(edited, ctx, _frame()))
    finally:
        md.close()


# ---- 11. temporal accumulation ----------------------------------------------------------------------------------------------------------------
def test_the_accumulator_drops_its_history_at_an_edit(ctx):
    sc = r.scene.make_random_scene(NX, NY, 3, False)
    flat, own = fl.flatten(sc), sc["camera"]
    edited = _edit(flat, _sphere_edit)
    views = cam.orbit(own, 120)[:3]  # 3 degrees apart
    seed = 77
    live = core.DeviceScene(flat, ctx=ctx)
    try:
        acc = core.TemporalAccumulator(live, NX, NY, NS, seed=seed)
        assert acc.step(views[0])[4] == 0.0
        assert acc.step(views[1])[4] > 0.0
        lin, q, se, w, share = acc.step(views[2], materials=edited)
        assert share == 0.0 and (w.cpu().numpy() == NS).all()
        own_frame = _fresh(_with_camera(edited, views[2]), ctx, lambda ds: ds.render_progressive(NX, NY, 0, NS, core.DEFAULT_DEPTH, seed + 2))
        assert np.array_equal(lin.cpu().numpy(), own_frame[0]) and np.array_equal(q.cpu().numpy(), own_frame[1])
        assert np.array_equal(se.cpu().numpy(), own_frame[2], equal_nan=True) and np.array_equal(acc.rays, own_frame[3])
        assert acc.step(views[1])[4] > 0.0  # the step after it takes history again
    finally:
        ctx.progressive_release()
        live.close()
