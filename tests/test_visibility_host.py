"""Closest-hit / any-hit queries, the parts that need no GPU: the C-ABI's prototypes and argument checks, camera.hemisphere_rays, the ray DeviceScene.pick
sends, and the condition of the GPU suite's traversal-count test (tests/test_gpu_visibility.py: "the exit is real")."""
import ctypes as C
import os
import re

import numpy as np

from raytrace_clj_amd import _ffi, camera, core, util
from tests import visibility_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtmi_query_hits", "rtmi_query_hits_device", "rtmi_query_occluded", "rtmi_query_occluded_device")
E_ARG, E_STATE = -1, -5


def _lib():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    return _ffi.lib()


def _prototypes():
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\bint\s+(rtmi_query_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_four_entries_and_ffi_binds_them():
    protos = _prototypes()
    assert sorted(protos) == sorted(ENTRIES)
    assert len(protos["rtmi_query_hits"]) == 11 and len(protos["rtmi_query_hits_device"]) == 12
    assert len(protos["rtmi_query_occluded"]) == 13 and len(protos["rtmi_query_occluded_device"]) == 14
    for name in ENTRIES:
        assert protos[name][0].startswith("rtmi_scene") and name in _ffi.SYMBOLS
        if name.endswith("_device"):
            assert protos[name][-1].replace(" ", "") == "void*stream"
    assert re.search(r"#define\s+RTMI_HIT_REC\s+12\b", open(os.path.join(ROOT, "include", "rtmi.h")).read()) and _ffi.HIT_REC == 12
    L = _lib()
    for name in ENTRIES:
        assert len(getattr(L, name).argtypes) == len(protos[name]), name
    assert L.rtmi_version() >= 216


def test_argument_errors_come_before_the_handle():
    L = _lib()
    rays, out, cnt = np.zeros((4, 7)), np.zeros((4, 12)), np.zeros(2, np.uint64)
    p = _ffi.ptr
    big = 2 ** 31 - 63  # one more than the 2^31 - 64 rays a call may hold
    hits = lambda n, r, o: L.rtmi_query_hits(None, 0, n, r, None, 0.001, 1.0, None, 0, o, p(cnt))  # noqa: E731
    hits_d = lambda n, r, o: L.rtmi_query_hits_device(None, 0, n, r, None, 0.001, 1.0, None, 0, o, None, None)  # noqa: E731
    occ = lambda ng, g, r: L.rtmi_query_occluded(None, 0, ng, g, r, None, 0.001, 1.0, None, 0, None, None, p(cnt))  # noqa: E731
    occ_d = lambda ng, g, r: L.rtmi_query_occluded_device(None, 0, ng, g, r, None, 0.001, 1.0, None, 0, None, None, None, None)  # noqa: E731
    for f in (hits, hits_d):
        assert f(-1, p(rays), p(out)) == E_ARG          # n < 0
        assert f(4, None, p(out)) == E_ARG              # NULL rays
        assert f(4, p(rays), None) == E_ARG             # NULL out_hits
        assert f(big, p(rays), p(out)) == E_ARG         # an overflowing n
    for f in (occ, occ_d):
        assert f(-1, 1, p(rays)) == E_ARG               # n_groups < 0
        assert f(4, 0, p(rays)) == E_ARG                # group <= 0
        assert f(4, -3, p(rays)) == E_ARG
        assert f(4, 1, None) == E_ARG                   # NULL rays
        assert f(2 ** 30, 4, p(rays)) == E_ARG          # n_groups * group overflows
        assert f(1, big, p(rays)) == E_ARG
    # with sound arguments the NULL handle is what is wrong: RTMI_E_STATE, not RTMI_E_ARG
    assert hits(4, p(rays), p(out)) == E_STATE and occ(4, 1, p(rays)) == E_STATE


# ---- camera.hemisphere_rays -----------------------------------------------------------------------------------------------------------------
def _points_normals(n, seed=3):
    rng = np.random.default_rng(seed)
    normals = rng.normal(0, 1, (n, 3)) * rng.uniform(0.1, 4.0, (n, 1))  # any length
    normals[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)  # the frame's special cases
    return rng.normal(0, 5, (n, 3)), normals


def test_hemisphere_rays_are_unit_and_on_the_normals_side():
    p, n = _points_normals(500)
    rays = camera.hemisphere_rays(p, n, 16, time=0.25)
    assert rays.shape == (500 * 16, 7) and rays.dtype == np.float64
    assert np.array_equal(rays[:, 0:3], np.repeat(p, 16, axis=0)) and np.all(rays[:, 6] == 0.25)
    d = rays[:, 3:6]
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-14
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    assert ((np.repeat(unit, 16, axis=0) * d).sum(axis=1) >= 0.0).all()


def test_hemisphere_rays_do_not_depend_on_the_split_over_first():
    p, n = _points_normals(64)
    whole = camera.hemisphere_rays(p, n, 12, seed=99).reshape(64, 12, 7)
    for cut in (1, 5, 11):
        a = camera.hemisphere_rays(p, n, cut, first=0, seed=99).reshape(64, cut, 7)
        b = camera.hemisphere_rays(p, n, 12 - cut, first=cut, seed=99).reshape(64, 12 - cut, 7)
        assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    assert not np.array_equal(camera.hemisphere_rays(p, n, 12, seed=100).reshape(64, 12, 7), whole)
    # the stream: ray r of point g takes draws 0 and 1 of sample_key(seed, g, first + r)
    g, r = 7, 4
    key = util.sample_key(99, g, r)
    xi0 = (util.draw_bits(key, 0) >> 11) * 2.0 ** -53
    unit = n[g] / np.linalg.norm(n[g])
    assert abs(float(whole[g, r, 3:6] @ unit) - np.sqrt(1.0 - xi0)) < 1e-14


def test_hemisphere_rays_are_cosine_weighted():
    """E[n . d] of a cosine-weighted hemisphere is 2/3 (a uniform one gives 1/2); the mean of 10^5 draws has a standard deviation of 7.5e-4"""
    p, n = _points_normals(1000)
    rays = camera.hemisphere_rays(p, n, 100)
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    cos = (np.repeat(unit, 100, axis=0) * rays[:, 3:6]).sum(axis=1)
    assert len(cos) == 100000 and abs(float(cos.mean()) - 2.0 / 3.0) < 0.01


# ---- DeviceScene.pick's ray ---------------------------------------------------------------------------------------------------------------
def test_pick_ray_is_the_oracles_camera_ray_at_the_pixel_centre(oracle):
    f = vc.flat("cloud(129)")  # a pinhole camera
    assert int(f.cam_kind) == 0
    nx, ny = 48, 40
    ds = object.__new__(core.DeviceScene)  # pixel_centre_rays reads the camera record only
    ds.camera_info = lambda: {"cam_kind": int(f.cam_kind), "cam": np.asarray(f.cam, np.float64)}
    cols, rows = np.array([0, 47, 13, 24, 5]), np.array([0, 39, 7, 20, 39])
    got = ds.pixel_centre_rays(nx, ny, cols, rows)
    uv = np.stack([(cols + 0.5) / nx, ((ny - 1 - rows) + 0.5) / ny], axis=1)
    exp = oracle.probe_camera(f, uv, np.zeros(len(uv), np.uint64))[:, :7]
    assert np.array_equal(got, exp)
    every = ds.pixel_centre_rays(nx, ny)
    assert every.shape == (nx * ny, 7) and np.array_equal(every[rows * nx + cols], got)  # row-major from the top


# ---- the condition of the traversal-count test ------------------------------------------------------------------------------------------------
def test_count_rays_mostly_hit(oracle):
    """the GPU suite compares the work of the any-hit and the closest-hit search on these rays: that says something only if most of them hit"""
    rays = vc.count_rays(oracle)
    assert rays.shape == (vc.N, 7) and np.isfinite(rays).all()
    h = oracle.probe_hit(vc.count_flat(), rays, tmin=0.001, tmax=vc.FLT_MAX)
    share = float((h[:, 0] == 1).mean())
    print("count rays that hit: %.3f" % share)
    assert share >= 0.5


def test_ray_sets_have_the_promised_shape(oracle):
    for name in ("cover", "cloud(129)", "chain(1000, 0.9, 0.15)"):
        rays = vc.rays(oracle, name)
        assert rays.shape == (vc.N, 7) and vc.N % 64 != 0 and (vc.N + 63) // 64 == 47
    assert (vc.rays(oracle, "cover")[:, 6] > 1.0).any() and (vc.rays(oracle, "cover")[:, 6] <= 1.0).any()
