"""Direct lighting from first hits (rtmi_scene_lights, rtmi_direct_irradiance*, rtmi_render_direct*), the parts that need no GPU: which primitives are
lights (rtmi_test_scene_lights against the header's rule), the numpy restatement of the light rule (camera.light_samples, tests/direct_reference.py)
against closed forms, its fold over splits, the C-ABI's prototypes and argument checks, and -- with the CPU oracle -- that the points the GPU tests
take from every scene really exercise what those tests claim."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

from raytrace_clj_amd import _ffi, camera
from raytrace_clj_amd import flatten as fl
from tests import direct_cases as dcs
from tests import direct_reference as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtmi_direct_irradiance", "rtmi_direct_irradiance_device", "rtmi_render_direct", "rtmi_render_direct_device")
E_ARG, E_STATE = -1, -5
N_MC = 4096  # samples of the closed-form checks


def _lib():
    return _ffi.lib()


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


# ---- which primitives are lights ---------------------------------------------------------------------------------------------------------------
def _lights(f, capacity=64):
    """rtmi_test_scene_lights over a FlatScene -> (the listed primitives, the count)"""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    kind, geom, mat = i32(f.prim_kind), np.ascontiguousarray(f.prim_geom, np.float64), i32(f.prim_mat)
    mat_kind, mat_tex, tex_kind = i32(f.mat_kind), i32(f.mat_tex), i32(f.tex_kind)
    chains = getattr(f, "prim_xform", None)
    chains = i32(chains) if chains is not None and len(chains) == len(kind) else None
    out, count = np.full(max(capacity, 1), -1, np.int32), ctypes.c_int32(-1)
    p = _ffi.ptr
    rc = _lib().rtmi_test_scene_lights(len(kind), p(kind), p(geom), p(mat), len(mat_kind), p(mat_kind), p(mat_tex), len(tex_kind), p(tex_kind), p(chains),
                                       capacity, p(out) if capacity else None, ctypes.byref(count))
    assert rc == 0, _lib().rtmi_last_error()
    return out[:min(count.value, capacity)].tolist(), count.value


def test_the_lights_of_the_reference_scenes():
    import raytrace_clj_amd as r
    f = dcs.flat("example-light")
    lights, count = _lights(f)
    assert count == 2 and lights == sorted(lights) == dref.eligible(f).tolist()
    assert sorted(int(f.prim_kind[i]) for i in lights) == [0, 3]  # its sphere and its rect_xy
    f = dcs.flat("cornell")
    lights, count = _lights(f)
    assert count == 1 and int(f.prim_kind[lights[0]]) == 4
    assert np.asarray(f.prim_geom, np.float64).reshape(-1, 9)[lights[0], :5].tolist() == [213.0, 227.0, 343.0, 332.0, 554.0]  # its one rect_xz
    f = fl.flatten(r.scene.make_random_scene(40, 24, 11, True))  # the cover scene: its dome is a gradient
    assert 3 in [int(k) for k in f.mat_kind] and _lights(f) == ([], 0)
    f = dcs.flat("two-triangles")
    lights, count = _lights(f)
    assert count == 1 and int(f.prim_kind[lights[0]]) == 0 and np.asarray(f.prim_geom, np.float64).reshape(-1, 9)[lights[0], 3] == 1000.0  # its constant dome
    assert _lights(dcs.flat("sphere-lamp"))[0] == dref.eligible(dcs.flat("sphere-lamp")).tolist() == [6]


def test_what_is_not_a_light():
    cases = dcs.not_lights()
    assert sorted(cases) == ["boundary", "moving", "translated", "zero-extent", "zero-radius"]
    for name, f in cases.items():
        assert 3 in [int(f.mat_kind[m]) for m in f.prim_mat], name  # an emitter is there ...
        assert _lights(f) == ([], 0), name                           # ... and is left out, without an error
        assert len(dref.eligible(f)) == 0, name
    assert int(cases["translated"].prim_xform[-1][1]) == 1 and int(cases["moving"].prim_kind[-1]) == 2 and int(cases["boundary"].prim_kind[-1]) == 16
    # a gradient emitter, and a lamp whose material index is out of range
    import copy
    f = copy.copy(dcs.flat("sphere-lamp"))
    f.tex_kind = np.array(f.tex_kind, np.int32)
    f.tex_kind[int(f.mat_tex[int(f.prim_mat[6])])] = 1
    assert _lights(f) == ([], 0)
    f = copy.copy(dcs.flat("sphere-lamp"))
    f.prim_mat = np.array(f.prim_mat, np.int32)
    f.prim_mat[6] = 99
    assert _lights(f) == ([], 0)


def test_capacity_and_argument_checks_of_the_list():
    f = dcs.flat("example-light")
    assert _lights(f, capacity=1) == ([2], 2) and _lights(f, capacity=0) == ([], 2)
    L, count = _lib(), ctypes.c_int32(0)
    out = np.zeros(4, np.int32)
    assert L.rtmi_test_scene_lights(0, None, None, None, 0, None, None, 0, None, None, 4, _ffi.ptr(out), ctypes.byref(count)) == 0 and count.value == 0
    assert L.rtmi_test_scene_lights(0, None, None, None, 0, None, None, 0, None, None, -1, _ffi.ptr(out), ctypes.byref(count)) == E_ARG
    assert L.rtmi_test_scene_lights(0, None, None, None, 0, None, None, 0, None, None, 4, None, ctypes.byref(count)) == E_ARG
    assert L.rtmi_test_scene_lights(0, None, None, None, 0, None, None, 0, None, None, 4, _ffi.ptr(out), None) == E_ARG
    assert L.rtmi_test_scene_lights(3, None, None, None, 0, None, None, 0, None, None, 4, _ffi.ptr(out), ctypes.byref(count)) == E_ARG
    assert L.rtmi_scene_lights(None, 4, _ffi.ptr(out), ctypes.byref(count)) == E_STATE
    assert L.rtmi_scene_lights(None, -1, _ffi.ptr(out), ctypes.byref(count)) == E_ARG


def test_light_table():
    f = dcs.flat("example-light")
    t = camera.light_table(f, [2, 3])
    assert t.shape == (2, camera.LIGHT_REC)
    assert t[0].tolist() == [3.0, 3.0, 1.0, 5.0, 3.0, -2.0, 4.0, 4.0, 4.0, 4.0]  # rect_xy 3..5 x 1..3 at z = -2: area 4, Le 4
    assert t[1].tolist() == [0.0, 0.0, 7.0, 0.0, 2.0, 0.0, camera.FOURPI * 4.0, 4.0, 4.0, 4.0]
    assert camera.FOURPI == 4.0 * math.pi and dref.INV_PI == 1.0 / math.pi


# ---- the restatement against closed forms (no occluders) -----------------------------------------------------------------------------------------
def _record(p, n, mat=0):
    return np.array([[1.0, 0.0, 1.0, p[0], p[1], p[2], n[0], n[1], n[2], 0.0, 0.0, float(mat)]])


def _estimate(rec, lights, seed):
    """-> (mean, standard error) of the restatement's per-sample values of channel 0, N_MC samples"""
    rays, w, built = dref.light_items(rec, lights, N_MC, seed=seed)
    c = dref.contributions(w, built, np.zeros(len(w), np.uint8), lights)
    per_sample = c[:, 0].reshape(N_MC, len(lights)).sum(axis=1)
    E, _ = dref.fold(c, 1, N_MC)
    mean = per_sample.mean()
    assert abs(E[0, 0] - mean) <= 1e-12 * abs(mean)  # the fold is that mean
    return mean, per_sample.std(ddof=1) / math.sqrt(N_MC), built


def _corner(a, b, h):
    """form factor from a differential element to a parallel rectangle a x b at height h with one corner above the element"""
    ra, rb = math.sqrt(a * a + h * h), math.sqrt(b * b + h * h)
    return (a / ra * math.atan(b / ra) + b / rb * math.atan(a / rb)) / (2.0 * math.pi)


def _rect_form_factor(x0, z0, x1, z1, h):
    signed = lambda a, b: math.copysign(1.0, a) * math.copysign(1.0, b) * _corner(abs(a), abs(b), h) if a and b else 0.0  # noqa: E731
    return signed(x1, z1) - signed(x0, z1) - signed(x1, z0) + signed(x0, z0)


@pytest.mark.parametrize("rect", [(-1.0, -2.0, 3.0, 1.5, 2.0), (0.5, 0.25, 2.0, 3.0, 1.0), (-2.0, -2.0, 2.0, 2.0, 0.5)])
def test_a_point_under_a_parallel_rectangle(rect):
    x0, z0, x1, z1, h = rect
    le = 3.0
    light = np.array([[4.0, x0, z0, x1, z1, h, abs((x1 - x0) * (z1 - z0)), le, 0.5, 0.25]])
    mean, se, built = _estimate(_record((0, 0, 0), (0, 2.0, 0)), light, seed=101)  # (a normal of length 2: the rule normalises it)
    exact = math.pi * le * _rect_form_factor(x0, z0, x1, z1, h)
    print("rectangle %s: estimate %.6f +- %.6f, closed form %.6f" % (rect, mean, se, exact))
    assert built.all() and se > 0.0 and abs(mean - exact) <= 5.0 * se


@pytest.mark.parametrize("r,D", [(1.0, 3.0), (0.5, 0.75), (2.0, 40.0)])
def test_a_point_facing_a_sphere_light(r, D):
    le = 2.5
    light = np.array([[0.0, 1.0, 2.0 + D, -1.0, r, 0.0, camera.FOURPI * (r * r), le, 1.0, 1.0]])
    mean, se, built = _estimate(_record((1.0, 2.0, -1.0), (0, 1, 0)), light, seed=202)
    exact = math.pi * le * (r / D) ** 2
    print("sphere r %g D %g: estimate %.6f +- %.6f, closed form %.6f, built %.3f" % (r, D, mean, se, exact, built.mean()))
    assert 0.0 < built.mean() < 1.0  # the far side builds no ray
    assert abs(built.mean() - 0.5 * (1.0 - r / D)) < 0.05  # the cap seen from outside: (1 - r / D) / 2 of the sphere's area
    assert abs(mean - exact) <= 5.0 * se


@pytest.mark.parametrize("p,n", [((0, 0, 0), (0, 1, 0)), ((3.0, -2.0, 5.0), (1.0, 1.0, -0.5))])
def test_a_point_inside_a_constant_dome(p, n):
    le = 0.4
    light = np.array([[1.0, 0.0, 0.0, 0.0, 10.0, 0.0, camera.FOURPI * 100.0, le, le, le]])
    mean, se, built = _estimate(_record(p, n), light, seed=303)
    print("dome from %s: estimate %.6f +- %.6f, closed form %.6f" % (p, mean, se, math.pi * le))
    assert 0.2 < built.mean() < 0.8  # the half below the point's horizon builds no ray; nothing is culled as a far side
    assert abs(mean - math.pi * le) <= 5.0 * se


def test_samples_lie_on_the_lights_and_weights_are_the_geometry_term():
    lights = camera.light_table(dcs.flat("example-light"), [2, 3])
    rng = np.random.default_rng(5)
    p, n = rng.normal(0, 3, (200, 3)) + (0.0, 3.0, 0.0), rng.normal(0, 1, (200, 3))
    rays, w, built = camera.light_samples(p, n, lights, 6, first=2, seed=9, time=0.5)
    assert rays.shape == (200 * 6 * 2, 7) and built.any() and (~built).any()
    q = rays[:, 0:3] + rays[:, 3:6]
    l = np.arange(len(rays)) % 2
    rect, sph = built & (l == 0), built & (l == 1)
    assert np.all(np.abs(q[rect, 2] + 2.0) < 1e-12) and np.all((q[rect, 0] >= 3) & (q[rect, 0] <= 5) & (q[rect, 1] >= 1) & (q[rect, 1] <= 3))
    assert np.allclose(np.sqrt(((q[sph] - (0, 7, 0)) ** 2).sum(axis=1)), 2.0, rtol=0, atol=1e-12)
    assert np.all(rays[built, 6] == 0.5) and not rays[~built].any() and not w[~built].any() and (w[built] > 0).all()
    # splits over `first` give the items of one call
    a = camera.light_samples(p, n, lights, 2, first=2, seed=9, time=0.5)
    b = camera.light_samples(p, n, lights, 4, first=4, seed=9, time=0.5)
    both = np.concatenate([a[0].reshape(200, 2, 2, 7), b[0].reshape(200, 4, 2, 7)], axis=1)
    assert np.array_equal(both.view(np.uint64), rays.reshape(200, 6, 2, 7).view(np.uint64))


# ---- the fold ----------------------------------------------------------------------------------------------------------------------------------
def test_fold_splits_equal_one_call():
    lights = camera.light_table(dcs.flat("example-light"), [2, 3])
    rng = np.random.default_rng(8)
    rec = np.zeros((50, 12))
    rec[:, 0], rec[:, 3:6], rec[:, 6:9] = 1.0, rng.normal(0, 2, (50, 3)) + (2.0, 3.0, 0.0), rng.normal(0, 1, (50, 3))
    one = dref.light_items(rec, lights, 7, seed=4)
    flags = (rng.random(len(one[1])) < 0.3).astype(np.uint8)
    c = dref.contributions(one[1], one[2], flags, lights)
    E, state = dref.fold(c, 50, 7)
    assert (E != 0).any() and (state[:, 3] == 7).all()
    by_chunk = flags.reshape(50, 7, 2)
    for split in ((3, 4), (1, 1, 5), (6, 1)):
        st, first = np.zeros((50, 4)), 0
        for n in split:
            part = dref.light_items(rec, lights, n, first=first, seed=4)
            cc = dref.contributions(part[1], part[2], np.ascontiguousarray(by_chunk[:, first:first + n]).ravel(), lights)
            Es, st = dref.fold(cc, 50, n, first=first, state=st)
            first += n
        assert np.array_equal(Es.view(np.uint64), E.view(np.uint64)) and np.array_equal(st.view(np.uint64), state.view(np.uint64)), split
    # the sum starts FROM the first item: a point whose only contribution is -0.0 keeps it (0 + -0.0 would be +0.0)
    E0, _ = dref.fold(np.array([[-0.0, 1.0, 2.0]]), 1, 1)
    assert math.copysign(1.0, E0[0, 0]) == -1.0


# ---- the points the GPU tests take from every scene ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dcs.SCENES)
def test_points_exercise_the_rule(name):
    """From the oracle's first hits of the view rays (and direct_cases.place's points): some items build no ray, some rays are free, some are occluded.
    In make_two_triangles the scene's own first hits cannot be occluded -- its two triangles are coplanar, and a ray between two points of the dome
    meets a triangle with probability about 1e-7 --, which is what the placed points are for."""
    f = dcs.flat(name)
    view = dcs.view_rays(_oracle(), name)
    rec = dcs.oracle_records(_oracle(), name, view)
    lights = camera.light_table(f, dref.eligible(f))
    if name == "two-triangles":
        own = dref.light_items(rec, lights, 5, view=view, seed=77)
        assert not _oracle().probe_hit(f, np.ascontiguousarray(own[0][own[2]]), tmin=0.001, tmax=1.0 - 0.001)[:, 0].any()
    rec, view = dcs.place(name, rec, view)
    rays, w, built = dref.light_items(rec, lights, 64, view=view, seed=77)  # (the seed and one of the sample counts of the GPU tests)
    assert 0 < built.sum() < len(built)
    flags = _oracle().probe_hit(f, np.ascontiguousarray(rays[built]), tmin=0.001, tmax=1.0 - 0.001)[:, 0]
    print("%s: %d items, %d built, %d occluded" % (name, len(built), built.sum(), int(flags.sum())))
    assert (flags == 0).any() and (flags == 1).any()
    if name == "two-triangles":
        e = rec[:, 3:6] - lights[0, 1:4]
        assert ((e * e).sum(axis=1)[rec[:, 0] == 1] <= 1000.0 ** 2 * (1 + 1e-12)).all()  # every point is inside (or on) its light
    lamb = dref.light_items(rec, lights, 64, view=view, seed=77, lambert_only=True, mat_kind=f.mat_kind)[2]
    assert not (lamb & ~built).any() and 0 < lamb.sum()
    # emitters, metal and glass build nothing under lambert_only (a point of the Cornell lamp builds no ray towards its own plane either way)
    assert lamb.sum() < built.sum() or name == "cornell"


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------------------
def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(rtmi_(?:direct|render_direct|scene_lights|test_scene_lights)\w*)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_entries_and_the_library_exports_them():
    protos = _prototypes()
    assert sorted(protos) == sorted(ENTRIES + ("rtmi_scene_lights", "rtmi_test_scene_lights"))
    assert len(protos["rtmi_direct_irradiance"]) == 18 and len(protos["rtmi_render_direct"]) == 12 and len(protos["rtmi_scene_lights"]) == 4
    L = _lib()
    for name in protos:
        assert name in _ffi.SYMBOLS and len(getattr(L, name).argtypes) == len(protos[name]), name
        if name.endswith("_device"):
            assert protos[name][-1].replace(" ", "") == "void*stream" and len(protos[name]) == len(protos[name[:-7]]) + 1
    assert L.rtmi_version() >= 218
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "THE LIGHT RULE" in header and "RTMI_DIRECT_REC 4" in header and "RTMI_DIRECT_MAX_LIGHTS 32" in header
    assert _ffi.DIRECT_REC == 4 and _ffi.DIRECT_MAX_LIGHTS == 32


def test_argument_errors_come_before_the_handle():
    L, p = _lib(), _ffi.ptr
    hits, E, cnt, lights = np.zeros((4, 12)), np.zeros((4, 3)), np.zeros(2, np.uint64), np.zeros(40, np.int32)
    di = lambda n, h, nl, lp, ns, first, out: L.rtmi_direct_irradiance(None, 0, n, h, None, nl, lp, ns, first, 1, 0.0, 0, None, out, None, None, None, p(cnt))  # noqa: E731
    di_d = lambda n, h, nl, lp, ns, first, out: L.rtmi_direct_irradiance_device(None, 0, n, h, None, nl, lp, ns, first, 1, 0.0, 0, None, out, None, None, None, None, None)  # noqa: E731
    for f in (di, di_d):
        assert f(-1, p(hits), 1, p(lights), 2, 0, p(E)) == E_ARG   # n_points < 0
        assert f(4, p(hits), 1, p(lights), 0, 0, p(E)) == E_ARG    # n_samples <= 0
        assert f(4, p(hits), 1, p(lights), 2, -1, p(E)) == E_ARG   # first < 0
        assert f(4, p(hits), -1, p(lights), 2, 0, p(E)) == E_ARG   # n_lights < 0
        assert f(4, p(hits), 33, p(lights), 2, 0, p(E)) == E_ARG   # 33 lights
        assert f(4, None, 1, p(lights), 2, 0, p(E)) == E_ARG       # NULL hits
        assert f(4, p(hits), 1, p(lights), 2, 0, None) == E_ARG    # NULL out_irradiance
        assert f(4, p(hits), 32, p(lights), 2, 0, p(E)) == E_STATE  # sound arguments: the NULL handle is what is wrong
        assert f(4, p(hits), 33, None, 2, 0, p(E)) == E_STATE      # without a list n_lights is not read
    lin = np.zeros((16, 3))
    rd = lambda nx, ny, ns, first, out: L.rtmi_render_direct(None, 0, nx, ny, ns, first, 1, None, out, None, None, p(cnt))  # noqa: E731
    rd_d = lambda nx, ny, ns, first, out: L.rtmi_render_direct_device(None, 0, nx, ny, ns, first, 1, None, out, None, None, None, None)  # noqa: E731
    for f in (rd, rd_d):
        assert f(-4, 4, 2, 0, p(lin)) == E_ARG
        assert f(4, 4, 0, 0, p(lin)) == E_ARG       # n_samples <= 0
        assert f(4, 4, 2, -1, p(lin)) == E_ARG      # first < 0
        assert f(4, 4, 2, 0, None) == E_ARG         # NULL out_linear
        assert f(2 ** 16, 2 ** 16, 1, 0, p(lin)) == E_ARG  # nx * ny beyond 2^31 - 64
        assert f(4, 4, 2, 0, p(lin)) == E_STATE


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_direct():
    from raytrace_clj_amd import core
    assert core._direct_flags(["out.png", "--direct", "8", "40"]) == (["out.png", "40"], 8)
    assert core._direct_flags(["--direct=4", "out.png"]) == (["out.png"], 4)
    assert core._direct_flags(["out.png", "40", "20"]) == (["out.png", "40", "20"], None)
    assert core._direct_name("a/b.png") == "a/b.direct.png"
    for bad in (["--direct"], ["--direct", "x"], ["--direct", "0"], ["--direct=-3"]):
        with pytest.raises(SystemExit) as e:
            core._direct_flags(bad)
        assert "--direct" in str(e.value)
    with pytest.raises(SystemExit) as e:
        core.main(["--direct", "4", "--panorama", "out.png"])
    assert "--direct does not combine" in str(e.value)
