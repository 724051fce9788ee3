"""CPU tests of the live scene's materials (rtmi_scene_set_materials, rtmi_scene_set_materials_stream): the C-ABI declares, binds and exports
them, the argument errors answer without a device and before the handle is examined, the Python hosts reject an edit with another primitive
count before they touch the library, and the edit's packer produces the bytes creation's does (rtmi_test_pack_materials: one function packs the
eleven material tables for both, the hook reaches it on both ways)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi, core
from raytrace_clj_amd import flatten as fl
from test_clj_conformance import GPU_CLJ, check_calls, header_prototypes, is_list, map_values, read_forms, walk

RTMI_E_ARG, RTMI_E_UNSUPPORTED, RTMI_E_STATE = -1, -3, -5
NAMES = ("rtmi_scene_set_materials", "rtmi_scene_set_materials_stream", "rtmi_test_pack_materials")
TABLES = ["i32", "int[]", "int[]", "double[]", "i32", "int[]", "double[]", "int[]", "int[]"]  # n_mats + 3 arrays, n_tex + 3 arrays, prim_mat


def test_prototypes_parse_and_are_bound():
    protos = header_prototypes()
    assert protos["rtmi_scene_set_materials"] == ["handle"] + TABLES + ["int[]"]
    assert protos["rtmi_scene_set_materials_stream"] == ["handle"] + TABLES + ["device-pointer"]
    assert len(protos["rtmi_test_pack_materials"]) == len(protos["rtmi_scene_create_ex"]) + 1  # creation's arrays, a flag, two outputs for one
    assert set(NAMES) <= set(_ffi.SYMBOLS)
    assert _ffi.EDIT_STREAM_MAX_BYTES == 32768
    assert "#define RTMI_EDIT_STREAM_MAX_BYTES 32768" in open(os.path.join(os.path.dirname(GPU_CLJ), "..", "..", "..", "include", "rtmi.h")).read()


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 213


def _tables(n_mats=2, n_tex=2):
    return (np.zeros(n_mats, np.int32), np.zeros(n_mats, np.int32), np.zeros(n_mats, np.float64),
            np.zeros(n_tex, np.int32), np.zeros((n_tex, fl.TEX_STRIDE), np.float64), np.full((n_tex, 2), -1, np.int32))


def test_argument_errors_answer_without_a_device_and_before_the_handle():
    """the scene handle is NULL in every call: a NULL table or a negative count is RTMI_E_ARG all the same -- the arguments are judged first --
    and only with good arguments (prim_mat may be NULL) is the handle what is reported"""
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    p = _ffi.ptr
    rebuilt = ctypes.c_int32(7)
    mk, mt, mp, tk, tp, tc = _tables()
    pm = np.zeros(3, np.int32)
    forms = (lambda *a: L.rtmi_scene_set_materials(None, *a, ctypes.byref(rebuilt)),
             lambda *a: L.rtmi_scene_set_materials(None, *a, None),
             lambda *a: L.rtmi_scene_set_materials_stream(None, *a, None))
    for call in forms:
        for hole in range(3):  # each material array in turn is NULL
            arrs = [p(mk), p(mt), p(mp)]
            arrs[hole] = None
            assert call(2, *arrs, 2, p(tk), p(tp), p(tc), p(pm)) == RTMI_E_ARG and "material arrays" in err()
        for hole in range(3):
            arrs = [p(tk), p(tp), p(tc)]
            arrs[hole] = None
            assert call(2, p(mk), p(mt), p(mp), 2, *arrs, p(pm)) == RTMI_E_ARG and "texture arrays" in err()
        assert call(-1, p(mk), p(mt), p(mp), 2, p(tk), p(tp), p(tc), p(pm)) == RTMI_E_ARG and "negative" in err()
        assert call(2, p(mk), p(mt), p(mp), -2, p(tk), p(tp), p(tc), p(pm)) == RTMI_E_ARG and "negative" in err()
        # good arguments: now the handle is examined (before the tables' contents: kind 99 would be RTMI_E_UNSUPPORTED)
        assert call(2, p(mk), p(mt), p(mp), 2, p(tk), p(tp), p(tc), p(pm)) == RTMI_E_STATE and "scene" in err()
        assert call(2, p(mk), p(mt), p(mp), 2, p(tk), p(tp), p(tc), None) == RTMI_E_STATE and "scene" in err()
        bad = mk.copy()
        bad[0] = 99
        assert call(2, p(bad), p(mt), p(mp), 2, p(tk), p(tp), p(tc), p(pm)) == RTMI_E_STATE
        assert call(0, None, None, None, 0, None, None, None, None) == RTMI_E_STATE  # empty tables need no arrays
    assert rebuilt.value == 7  # a failing call writes nothing


class _Handle:
    """a DeviceScene that never met the library: any call through its handle would fail loudly"""
    def __init__(self, flat):
        self.flat, self.handle, self.ctx = flat, None, None


def test_set_materials_rejects_another_primitive_count_without_touching_the_library(monkeypatch):
    flat = fl.flatten(r.scene.make_two_spheres(36, 20))
    other = fl.flatten(r.scene.make_random_scene(36, 20, 1, False))
    assert len(other.prim_kind) != len(flat.prim_kind)
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was called"))
    ds = _Handle(flat)
    for stream in (None, 0):
        with pytest.raises(ValueError) as e:
            core.DeviceScene.set_materials(ds, other, stream=stream)
        assert str(len(other.prim_kind)) in str(e.value) and str(len(flat.prim_kind)) in str(e.value)
    with pytest.raises(ValueError):
        core.DeviceScene.set_materials(ds, r.scene.make_cornell_box(36, 20))  # a scene is flattened first, then counted
    assert ds.flat is flat


def test_python_hosts_expose_the_edit():
    from raytrace_clj_amd import dist
    assert list(inspect.signature(core.DeviceScene.set_materials).parameters) == ["self", "scene_or_flat", "stream"]
    assert inspect.signature(core.DeviceScene.set_materials).parameters["stream"].default is None
    assert list(inspect.signature(dist.MultiDevice.set_materials).parameters) == ["self", "scene_or_flat"]
    step = inspect.signature(core.TemporalAccumulator.step).parameters
    assert list(step)[:2] == ["self", "camera"] and step["materials"].default is None
    assert "history" in core.TemporalAccumulator.step.__doc__ and "materials" in core.TemporalAccumulator.step.__doc__


# ---- one packer: the edit's tables are creation's ---------------------------------------------------------------------------------------------
def _pack(flat, through_creation, prim_mat=None, geometry=True):
    """-> (hash of the eleven tables, [materials' share of has_ext, uses_perlin, max_image])"""
    a = lambda x, dt: np.ascontiguousarray(x, dt)
    n = len(flat.prim_kind)
    pk, pg = a(flat.prim_kind, np.int32), a(flat.prim_geom, np.float64)
    pm = a(flat.prim_mat if prim_mat is None else prim_mat, np.int32)
    mk, mt, mp = a(flat.mat_kind, np.int32), a(flat.mat_tex, np.int32), a(flat.mat_param, np.float64)
    tk, tp, tc = a(flat.tex_kind, np.int32), a(flat.tex_param, np.float64), a(flat.tex_child, np.int32)
    c24, flip, xf = a(flat.cam, np.float64), a(flat.prim_flip, np.int32), a(flat.prim_xform, np.int32)
    xk, xp = a(flat.xform_kind, np.int32), a(flat.xform_param, np.float64)
    h, facts = np.zeros(1, np.uint64), np.full(3, -7, np.int32)
    p = _ffi.ptr
    geo = (p(pg), int(flat.cam_kind), p(c24), p(flip), p(xf), len(xk), p(xk), p(xp)) if geometry else (None, 0, None, None, None, 0, None, None)
    rc = _ffi.lib().rtmi_test_pack_materials(n, p(pk), geo[0], p(pm), len(mk), p(mk), p(mt), p(mp), len(tk), p(tk), p(tp), p(tc), *geo[1:],
                                             int(through_creation), p(h), p(facts))
    return rc, int(h[0]), [int(v) for v in facts]


SCENES = {
    "cover": lambda: r.scene.make_random_scene(36, 20, 3, False),
    "cover-moving": lambda: r.scene.make_random_scene(36, 20, 3, True),
    "cornell": lambda: r.scene.make_cornell_box(36, 20),
    "cornell-fog": lambda: r.scene.make_cornell_box(36, 20, classic=False),         # Isotropic phase functions on media
    "earth": lambda: r.scene.make_textured_sphere(36, 20, r.scene.synthetic_earth(32, 16)),  # a UV-reading texture: FlipV over an ImageMap
    "two-spheres": lambda: r.scene.make_two_spheres(36, 20),                        # UVGradients that read u and v
    "perlin": lambda: r.scene.make_two_perlin_spheres(36, 20),
    "triangles": lambda: r.scene.make_two_triangles(36, 20),
}
FACTS = {"cover": [0, 0, -1], "cover-moving": [0, 0, -1], "cornell": [0, 0, -1], "cornell-fog": [1, 0, -1], "earth": [1, 0, 0],
         "two-spheres": [0, 0, -1], "perlin": [1, 1, -1], "triangles": [0, 0, -1]}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_edit_packs_what_creation_packs(name):
    flat = fl.flatten(SCENES[name]())
    rc0, h0, f0 = _pack(flat, 0)
    rc1, h1, f1 = _pack(flat, 1)
    assert (rc0, rc1) == (0, 0), _ffi.lib().rtmi_last_error().decode()
    assert h0 == h1 and f0 == f1 == FACTS[name]
    assert _pack(flat, 0, geometry=False) == (0, h0, f0)  # the edit's packer reads no geometry, no instancing and no camera


def test_the_hash_sees_every_kind_of_edit():
    """a colour, a fuzz, a dielectric's index (its 1/ri and r0 live in the record), a material's kind, a checker's scale, a texture index (the
    NEEDS_* bits of the primitives), the assignment: each changes the tables, on both ways alike"""
    import copy
    flat = fl.flatten(SCENES["cover"]())
    base = _pack(flat, 0)[1]
    seen = {base}

    def edited(change):
        f = copy.copy(flat)
        for name in ("mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child", "prim_mat"):
            setattr(f, name, getattr(flat, name).copy())
        change(f)
        (rc0, h0, f0), (rc1, h1, f1) = _pack(f, 0), _pack(f, 1)
        assert (rc0, rc1) == (0, 0) and h0 == h1 and f0 == f1
        assert h0 not in seen
        seen.add(h0)

    const = int(np.flatnonzero(flat.tex_kind == fl.TEX_CONSTANT)[0])
    metal = int(np.flatnonzero(flat.mat_kind == fl.MAT_METAL)[0])
    glass = int(np.flatnonzero(flat.mat_kind == fl.MAT_DIELECTRIC)[0])
    lamb = int(np.flatnonzero(flat.mat_kind == fl.MAT_LAMBERTIAN)[0])
    checker = int(np.flatnonzero(flat.tex_kind == fl.TEX_CHECKER)[0])
    grad = int(np.flatnonzero(flat.tex_kind == fl.TEX_UVGRADIENT)[0])
    edited(lambda f: f.tex_param.__setitem__((const, 1), 0.125))
    edited(lambda f: f.mat_param.__setitem__(metal, 0.75))
    edited(lambda f: f.mat_param.__setitem__(glass, 2.4))
    edited(lambda f: f.mat_kind.__setitem__(lamb, fl.MAT_METAL))
    edited(lambda f: f.tex_param.__setitem__((checker, 0), 3.0))
    edited(lambda f: f.mat_tex.__setitem__(int(np.flatnonzero(flat.mat_tex == grad)[0]), const))  # the sky dome's UVSphere stops reading uv
    edited(lambda f: f.prim_mat.__setitem__(slice(0, 2), flat.prim_mat[1::-1].copy()) if flat.prim_mat[0] != flat.prim_mat[1] else None)


def test_the_hook_applies_the_checks_of_its_path():
    import copy
    flat = fl.flatten(SCENES["cornell-fog"]())

    def broken(change):
        f = copy.copy(flat)
        for name in ("mat_kind", "mat_tex", "prim_mat", "tex_kind"):
            setattr(f, name, getattr(flat, name).copy())
        change(f)
        return _pack(f, 0)[0], _pack(f, 1)[0]

    medium = int(np.flatnonzero((flat.prim_kind & ~fl.PRIM_BOUNDARY) == fl.PRIM_MEDIUM)[0])
    assert broken(lambda f: f.mat_tex.__setitem__(0, len(flat.tex_kind))) == (RTMI_E_ARG, RTMI_E_ARG)
    assert broken(lambda f: f.mat_kind.__setitem__(int(flat.prim_mat[medium]), fl.MAT_LAMBERTIAN)) == (RTMI_E_ARG, RTMI_E_ARG)
    assert "RTMI_MAT_ISOTROPIC" in _ffi.lib().rtmi_last_error().decode()
    assert broken(lambda f: f.prim_mat.__setitem__(0, len(flat.mat_kind))) == (RTMI_E_ARG, RTMI_E_ARG)
    assert broken(lambda f: f.tex_kind.__setitem__(0, 99)) == (RTMI_E_UNSUPPORTED, RTMI_E_UNSUPPORTED)
    assert broken(lambda f: f.mat_kind.__setitem__(0, -1)) == (RTMI_E_UNSUPPORTED, RTMI_E_UNSUPPORTED)


# ---- the Clojure host -------------------------------------------------------------------------------------------------------------------------
def test_gpu_clj_set_materials_conforms_to_the_header():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "set-materials" in by_name
    flat = [f for f in forms if is_list(f, "defn") and f[2] == "flatten-scene"][0]
    maps = [f for f in walk(flat) if isinstance(f, list) and f[0] == "{" and any(x == ":prim-kind" for x in f[1:])]
    protos, flat_map = header_prototypes(), map_values(maps[0])
    calls = {x[2].strip('"') for x in walk(by_name["set-materials"]) if is_list(x, "call-int")}
    assert calls == {"rtmi_scene_set_materials"}  # the host form, like set-camera: a JNA host has no stream to order the other one on
    assert check_calls([by_name["set-materials"]], protos, flat_map, True, "gpu.clj") == 1
    assert "rtmi_scene_set_materials" not in {x[2].strip('"') for x in walk(by_name["create-scene!"]) if is_list(x, "call-int")}
