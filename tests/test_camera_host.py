"""CPU tests of the live scene's camera (rtmi_scene_set_camera, rtmi_scene_set_camera_stream, rtmi_scene_camera): the C-ABI declares, binds and
exports them, the argument errors that need no device answer without one and before the handle is examined, camera.rotate_y is a rigid turn
about the vertical axis, the CLI parses --orbit, and the Clojure host's set-camera / render-views call only what the header declares."""
import ctypes
import math
import os

import numpy as np
import pytest

from raytrace_clj_amd import _ffi
from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from test_clj_conformance import GPU_CLJ, check_calls, header_prototypes, is_list, map_values, read_forms, walk

RTMI_E_ARG, RTMI_E_UNSUPPORTED, RTMI_E_STATE = -1, -3, -5
NAMES = ("rtmi_scene_set_camera", "rtmi_scene_set_camera_stream", "rtmi_scene_camera")
FIELDS = ("origin", "lleft", "horiz", "vert", "u", "v", "w")


def _lens(aperture=0.3):
    return cam.thin_lens_camera(lookfrom=[13.0, 2.0, 3.0], lookat=[0.5, 0.25, -1.0], vup=[0.0, 1.0, 0.0], vfov=20.0, aspect=60.0 / 36.0,
                                aperture=aperture, focus_dist=10.0, t0=0.25, t1=0.75)


def _pinhole():
    return cam.pinhole_camera(lookfrom=[-4.0, 3.0, 9.0], lookat=[0.5, 0.25, -1.0], vup=[0.0, 1.0, 0.0], vfov=35.0, aspect=2.0)


def test_prototypes_parse_and_are_bound():
    protos = header_prototypes()
    assert protos["rtmi_scene_set_camera"] == ["handle", "i32", "double[]", "int[]"]
    assert protos["rtmi_scene_set_camera_stream"] == ["handle", "i32", "double[]", "device-pointer"]
    assert protos["rtmi_scene_camera"] == ["handle", "int[]", "double[]", "double[]", "double[]"]
    assert set(NAMES) <= set(_ffi.SYMBOLS)


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 210


def test_argument_errors_answer_without_a_device_and_before_the_handle():
    """the scene handle is NULL in every call: a NULL cam is RTMI_E_ARG and a camera kind outside pinhole / thin lens RTMI_E_UNSUPPORTED all
    the same -- the arguments are judged first -- and only with good arguments is the handle what is reported"""
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    c = np.zeros(24, np.float64)
    rebuilt = ctypes.c_int32(7)
    forms = (lambda kind, p: L.rtmi_scene_set_camera(None, kind, p, ctypes.byref(rebuilt)),
             lambda kind, p: L.rtmi_scene_set_camera(None, kind, p, None),
             lambda kind, p: L.rtmi_scene_set_camera_stream(None, kind, p, None))
    for call in forms:
        assert call(0, None) == RTMI_E_ARG and "cam" in err()
        assert call(5, None) == RTMI_E_ARG and "cam" in err()  # cam NULL is reported first
        for kind in (-1, 2, 5):
            assert call(kind, _ffi.ptr(c)) == RTMI_E_UNSUPPORTED and "camera kind %d" % kind in err()
        for kind in (0, 1):
            assert call(kind, _ffi.ptr(c)) == RTMI_E_STATE and "scene" in err()
        c[:] = np.nan  # non-finite values are no argument error: creation accepts them too
        assert call(1, _ffi.ptr(c)) == RTMI_E_STATE and "scene" in err()
        c[:] = 0.0
    assert rebuilt.value == 7  # a failing call writes nothing


def test_scene_camera_of_a_null_handle_is_a_state_error():
    L = _ffi.lib()
    kind, lo, hi = ctypes.c_int32(), ctypes.c_double(), ctypes.c_double()
    c = np.zeros(24, np.float64)
    assert L.rtmi_scene_camera(None, None, None, None, None) == RTMI_E_STATE and "scene" in L.rtmi_last_error().decode()
    assert L.rtmi_scene_camera(None, ctypes.byref(kind), _ffi.ptr(c), ctypes.byref(lo), ctypes.byref(hi)) == RTMI_E_STATE


@pytest.mark.parametrize("make", (_lens, _pinhole))
def test_rotate_y_by_zero_is_the_identity_bit_for_bit(make):
    c = make()
    pivot = np.array([0.3, -7.0, 1e-3])
    r = cam.rotate_y(c, 0.0, pivot)
    assert type(r) is type(c)
    for name in FIELDS:
        if hasattr(c, name):
            a, b = np.asarray(getattr(c, name), np.float64), getattr(r, name)
            assert b is not getattr(c, name) and a.tobytes() == np.asarray(b, np.float64).tobytes(), name
    if isinstance(c, cam.ThinLensCamera):
        assert (r.aperture, r.t0, r.t1) == (c.aperture, c.t0, c.t1)
    neg = cam.PinholeCamera(np.array([-0.0, 1.0, -0.0]), np.array([1.0, -0.0, 2.0]), np.zeros(3), np.zeros(3))
    assert cam.rotate_y(neg, 0.0, pivot).origin.tobytes() == neg.origin.tobytes()  # the sign of a zero survives too


@pytest.mark.parametrize("make", (_lens, _pinhole))
def test_three_thirds_of_a_turn_return_within_a_few_ulps(make):
    """With u = 2^-53 and L the length of the vector: one turn computes c x + s z from a sine and a cosine within an ulp of the true ones (a
    relative u each), two rounded products and a rounded sum: at most 2 u (|c x| + |s z|) + u |x'| <= 3 u L per component and turn, 9 u L over
    three.  The angle 2 pi / 3 itself is rounded by up to 2.1 u, so the three turns miss the full turn by 6.3 u: another 6.3 u L.  A point is
    taken to the pivot and back, two more roundings of at most u (|p - pivot| + |pivot|) each per turn.  In all under 16 u L for a vector and
    under 22 u |p - pivot| + 12 u |pivot| for a point; the test allows 32 u = 16 eps of L, and of |p - pivot| + |p| + |pivot|."""
    c = make()
    pivot = np.array([0.5, 0.25, -1.0])
    r = c
    for _ in range(3):
        r = cam.rotate_y(r, 2.0 * math.pi / 3.0, pivot)
    eps = np.finfo(np.float64).eps
    for name in FIELDS:
        if not hasattr(c, name):
            continue
        a, b = np.asarray(getattr(c, name), np.float64), np.asarray(getattr(r, name), np.float64)
        scale = np.linalg.norm(a - pivot) + np.linalg.norm(a) + np.linalg.norm(pivot) if name in ("origin", "lleft") else np.linalg.norm(a)
        assert np.max(np.abs(a - b)) <= 16 * eps * scale, (name, np.max(np.abs(a - b)) / (eps * scale))
        assert a[1] == b[1]  # the vertical component is never touched


@pytest.mark.parametrize("angle", (0.1, 1.0, 2.0 * math.pi / 3.0, -2.5, 1e-9))
def test_rotate_y_is_rigid(angle):
    """|horiz|, |vert| and horiz . vert are kept (to the rounding of the products and sums: a few eps of |horiz| |vert|), the points keep their
    distance from the pivot's axis and their height, and the view still looks along -w: lleft - origin keeps its components in the turned frame"""
    c = _lens()
    pivot = np.array([0.5, 0.25, -1.0])
    r = cam.rotate_y(c, angle, pivot)
    eps = np.finfo(np.float64).eps
    nh, nv = np.linalg.norm(c.horiz), np.linalg.norm(c.vert)
    assert abs(np.linalg.norm(r.horiz) - nh) <= 4 * eps * nh and abs(np.linalg.norm(r.vert) - nv) <= 4 * eps * nv
    assert abs(np.dot(r.horiz, r.vert) - np.dot(c.horiz, c.vert)) <= 8 * eps * nh * nv
    for name in ("origin", "lleft"):
        a, b = getattr(c, name) - pivot, getattr(r, name) - pivot
        assert a[1] == b[1] or abs(a[1] - b[1]) <= 2 * eps * (abs(getattr(c, name)[1]) + abs(pivot[1]))
        assert abs(math.hypot(a[0], a[2]) - math.hypot(b[0], b[2])) <= 8 * eps * (np.linalg.norm(a) + np.linalg.norm(pivot))
    d0, d1 = c.lleft - c.origin, r.lleft - r.origin
    for x, y in ((c.u, r.u), (c.v, r.v), (c.w, r.w)):
        assert abs(np.dot(d0, x) - np.dot(d1, y)) <= 64 * eps * (np.linalg.norm(c.origin) + np.linalg.norm(c.lleft) + np.linalg.norm(pivot))
    # a quarter turn about the origin's axis maps +x to -z (x' = c x + s z, z' = -s x + c z)
    q = cam.rotate_y(cam.PinholeCamera(np.array([1.0, 2.0, 0.0]), np.zeros(3), np.zeros(3), np.zeros(3)), math.pi / 2, np.zeros(3))
    assert abs(q.origin[0]) <= eps and q.origin[1] == 2.0 and abs(q.origin[2] + 1.0) <= eps


def test_flatten_camera_of_a_turned_record_keeps_the_kind():
    for make, kind in ((_lens, fl.CAM_THINLENS), (_pinhole, fl.CAM_PINHOLE)):
        c = make()
        r = cam.rotate_y(c, 0.7, cam.view_pivot(c))
        k, c24 = fl.flatten_camera(r)
        assert k == kind and c24.shape == (24,) and c24.dtype == np.float64
        assert np.array_equal(c24[0:3], r.origin) and np.array_equal(c24[6:9], r.horiz)
        if kind == fl.CAM_THINLENS:
            assert tuple(c24[21:24]) == (c.aperture, c.t0, c.t1)
        else:
            assert not c24[12:].any()
    with pytest.raises(TypeError):
        cam.rotate_y(object(), 0.5, np.zeros(3))


def test_orbit_views_and_pivot():
    """view 0 of an orbit is the camera itself; the default pivot is the centre of the image plane: for a lens focused on its look-at point that
    point itself (to the rounding of the constructor)"""
    lookat = np.array([0.5, 0.25, -1.0])
    lookfrom = np.array([13.0, 2.0, 3.0])
    c = cam.thin_lens_camera(lookfrom=lookfrom, lookat=lookat, vup=[0.0, 1.0, 0.0], vfov=20.0, aspect=2.0, aperture=0.1,
                             focus_dist=float(np.linalg.norm(lookfrom - lookat)), t0=0.0, t1=1.0)
    assert np.max(np.abs(cam.view_pivot(c) - lookat)) <= 1e-13
    views = cam.orbit(c, 4)
    assert len(views) == 4 and all(type(v) is cam.ThinLensCamera for v in views)
    assert views[0].origin.tobytes() == c.origin.tobytes() and views[0].lleft.tobytes() == c.lleft.tobytes()
    half = views[2]  # half a turn: the origin is mirrored through the pivot's axis
    assert np.max(np.abs((half.origin - lookat)[[0, 2]] + (c.origin - lookat)[[0, 2]])) <= 1e-12 and half.origin[1] == c.origin[1]


def test_orbit_flag_parses():
    assert core._orbit_flags(["out.png", "60", "36", "4", "--orbit", "8"]) == (["out.png", "60", "36", "4"], 8)
    assert core._orbit_flags(["--orbit=3", "out.png", "--denoise", "2"]) == (["out.png", "--denoise", "2"], 3)
    assert core._orbit_flags(["out.png"]) == (["out.png"], None)
    for bad in (["--orbit"], ["--orbit", "x"], ["--orbit", "0"], ["--orbit=-2"], ["--orbit", "4", "--chunk", "8"], ["--orbit", "4", "--adaptive=0.1"],
                ["--adaptive-denoised", "0.1", "--orbit", "2"], ["--orbit", "2", "--budget", "1"], ["--noise=0.1", "--orbit", "2"]):
        with pytest.raises(SystemExit):
            core._orbit_flags(bad)
    assert core._orbit_name("a/b.x.png", 7) == "a/b.x_007.png" and core._orbit_name("frame", 12) == "frame_012"
    assert core._denoised_name(core._orbit_name("a.png", 0)) == "a_000.denoised.png"


def test_python_hosts_expose_the_camera():
    from raytrace_clj_amd import dist
    import inspect
    for name in ("set_camera", "camera_info", "render_views"):
        assert callable(getattr(core.DeviceScene, name))
    assert list(inspect.signature(core.DeviceScene.set_camera).parameters) == ["self", "camera", "stream"]
    assert callable(dist.MultiDevice.set_camera)
    step = inspect.signature(dist.FramePipeline.step).parameters
    assert list(step)[:3] == ["self", "ns", "camera"] and step["camera"].default is None


def test_gpu_clj_set_camera_and_render_views_conform_to_the_header():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "set-camera" in by_name and "render-views" in by_name
    flat = [f for f in forms if is_list(f, "defn") and f[2] == "flatten-scene"][0]
    maps = [f for f in walk(flat) if isinstance(f, list) and f[0] == "{" and any(x == ":prim-kind" for x in f[1:])]
    protos, flat_map = header_prototypes(), map_values(maps[0])
    calls = lambda entry: {x[2].strip('"') for x in walk(by_name[entry]) if is_list(x, "call-int")}
    assert calls("set-camera") == {"rtmi_scene_set_camera"}
    assert calls("render-views") == {"rtmi_init", "rtmi_render", "rtmi_scene_destroy", "rtmi_shutdown"}
    uses = {x[1] for x in walk(by_name["render-views"]) if is_list(x)}
    assert {"create-scene!", "set-camera"} <= uses, "render-views builds ONE scene through create-scene! and moves its camera with set-camera"
    assert "rtmi_scene_set_camera" not in calls("create-scene!")
    # declared symbols, declared arity, coerced scalars, typed arrays
    assert check_calls([by_name["set-camera"]], protos, flat_map, True, "gpu.clj") == 1
    assert check_calls([by_name["render-views"]], protos, flat_map, True, "gpu.clj") == 4
