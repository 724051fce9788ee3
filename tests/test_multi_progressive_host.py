"""CPU tests of progressive / adaptive frames on several devices (rtmi_render_adaptive_tiles_device, rtmi_assemble_progressive_device,
rtmi_render_multi_adaptive*): the C-ABI declares, binds and exports them, the argument errors that need no device answer without one, the numpy
helper's dealing and padding agree with dist.py's, its record and assembly invert each other, and the Clojure host calls the new entry."""
import ctypes
import os

import numpy as np
import pytest

import adaptive_reference as ar
import multi_progressive_reference as mp
from raytrace_clj_amd import _ffi
from raytrace_clj_amd import dist
from test_clj_conformance import GPU_CLJ, check_calls, header_prototypes, is_list, map_values, read_forms, walk

RTMI_E_ARG, RTMI_E_STATE = -1, -5
NAMES = ("rtmi_render_adaptive_tiles_device", "rtmi_assemble_progressive_device", "rtmi_render_multi_adaptive", "rtmi_render_multi_adaptive_device")


def test_prototypes_parse_with_the_types_the_reader_knows():
    protos = header_prototypes()
    head = ["i32", "i32", "i32", "i32", "i32", "f64", "i32", "i64", "i32"]  # nx ny s_first s_count retire eps depth seed precision
    assert protos["rtmi_render_adaptive_tiles_device"] == ["handle"] + head + ["i32", "i32"] + ["device-pointer"] * 3
    assert protos["rtmi_assemble_progressive_device"] == ["handle", "i32", "i32", "i32", "i32"] + ["device-pointer"] * 6
    assert protos["rtmi_render_multi_adaptive"] == ["i32", "handle-array"] + head + ["double[]", "byte[]", "double[]", "int[]", "long[]"]
    assert protos["rtmi_render_multi_adaptive_device"] == ["i32", "handle-array"] + head + ["device-pointer"] * 5
    assert set(NAMES) <= set(_ffi.SYMBOLS)
    assert "#define RTMI_PROG_REC 5" in open(os.path.join(os.path.dirname(GPU_CLJ), "..", "..", "..", "include", "rtmi.h")).read()
    assert _ffi.PROG_REC == mp.REC == 5


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 209


def _tiles(L, s_first=0, s_count=2, retire=1, eps=0.1, tile_first=0, tile_stride=1):
    return L.rtmi_render_adaptive_tiles_device(None, 8, 8, s_first, s_count, retire, eps, 50, 1, 0, tile_first, tile_stride, None, None, None)


def _multi(L, n=1, s_first=0, s_count=2, retire=1, eps=0.1, device_form=False):
    arr = (ctypes.c_void_p * 1)(None)
    if device_form:
        return L.rtmi_render_multi_adaptive_device(n, arr, 8, 8, s_first, s_count, retire, eps, 50, 1, 0, None, None, None, None, None)
    return L.rtmi_render_multi_adaptive(n, arr, 8, 8, s_first, s_count, retire, eps, 50, 1, 0, None, None, None, None, None)


def test_argument_errors_answer_without_a_device():
    """every one of these is RTMI_E_ARG although the scene handle is NULL: the arguments are judged before the handle is examined"""
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    for bad in (dict(tile_stride=0), dict(tile_stride=-3), dict(tile_first=-1), dict(s_count=0), dict(s_count=-2), dict(s_first=-1), dict(retire=2),
                dict(retire=-1), dict(eps=-0.5), dict(eps=float("nan")), dict(eps=float("inf"))):
        assert _tiles(L, **bad) == RTMI_E_ARG and err(), bad
    assert "retire" in err() or "eps" in err()
    for device_form in (False, True):
        for bad in (dict(n=0), dict(n=-1)):
            assert _multi(L, device_form=device_form, **bad) == RTMI_E_ARG and err(), bad
    for bad in (dict(s_count=0), dict(retire=3), dict(eps=-1.0), dict(eps=float("nan"))):
        assert _multi(L, device_form=True, **bad) == RTMI_E_ARG and err(), bad
    # eps is not read with retire = 0: the same values pass the argument checks, and the NULL handle is what is reported
    for eps in (-0.5, float("nan"), float("inf")):
        assert _tiles(L, retire=0, eps=eps) == RTMI_E_STATE and "scene" in err()
    assert _tiles(L) == RTMI_E_STATE and "scene" in err()
    assert L.rtmi_assemble_progressive_device(None, 8, 8, 1, 1, None, None, None, None, None, None) == RTMI_E_STATE and "context" in err()


@pytest.mark.parametrize("world", mp.WORLDS)
def test_helper_dealing_and_padding_match_dist(world):
    nx, ny = mp.SIZE
    assert mp.n_tiles(nx, ny) == dist.n_tiles(nx, ny) == 15
    assert mp.per_rank(nx, ny, world) == dist.tiles_per_rank(nx, ny, world)
    seen = []
    for r in range(world):
        assert mp.local_tiles(nx, ny, r, world) == dist.local_tile_ids(nx, ny, r, world)
        seen += mp.local_tiles(nx, ny, r, world)
    assert sorted(seen) == list(range(15))


@pytest.mark.parametrize("world", mp.WORLDS)
def test_helper_records_and_assembly_invert_each_other(world):
    nx, ny = mp.SIZE
    rng = np.random.default_rng(world)
    linear, stderr = rng.random((ny, nx, 3)) + 0.25, rng.random((ny, nx)) + 0.25
    stderr[3, 5] = np.inf
    samples = rng.integers(1, 9, (ny, nx)).astype(np.int32)
    g = mp.gathered_records(linear, stderr, samples, world)
    per = mp.per_rank(nx, ny, world)
    assert g.shape == (world, per, 64, 5)
    lin, q, err, smp = mp.assemble(g, nx, ny)
    assert np.array_equal(lin, linear) and np.array_equal(err, stderr) and np.array_equal(smp, samples) and smp.dtype == np.int32
    # everything the frame does not cover is zero: padding slots and the out-of-image pixels of the edge tiles
    covered = np.zeros((world, per, 64), bool)
    for y in range(ny):
        for x in range(nx):
            t = (y // 8) * 5 + x // 8
            covered[t % world, t // world, (y % 8) * 8 + x % 8] = True
    assert covered.sum() == nx * ny and (g[~covered] == 0).all() and (g[covered][:, 4] >= 1).all()
    for r in range(world):  # the primitive's own buffer: the local tiles only, no padding
        own = mp.dealt_records(linear, stderr, samples, r, world)
        assert own.shape[0] == len(dist.local_tile_ids(nx, ny, r, world)) and np.array_equal(own, g[r, :own.shape[0]])


def test_helper_schedule_is_adaptive_reference_schedule_on_a_uniform_run():
    nx, ny = mp.SIZE
    rng = np.random.default_rng(7)
    level = ar.per_pixel(rng.random((3, 5)), nx, ny)  # a tile with level v retires once 4 v / k <= eps
    planes = {k: level * rng.uniform(0.9, 1.0, (ny, nx)) * (4.0 / k) for k in (4, 8, 12, 16)}
    planes[8][0, 0] = np.nan
    eps = 0.2
    ref = ar.schedule(lambda k: planes[k], nx, ny, 4, 4, 16, eps)
    got = mp.schedule_chunks(lambda k: planes[k], nx, ny, (4, 4, 4, 4), eps)
    assert len(ref) == len(got) == 4 and 0 < ref[-1][2].sum() < 15
    for (k, n_t, act, _), (k2, n_t2, act2) in zip(ref, got):
        assert k == k2 and np.array_equal(n_t, n_t2) and np.array_equal(act, act2)
    flat = mp.schedule_chunks(lambda k: planes[k], nx, ny, (4, 4, 4, 4), eps, retire=False)
    assert all(act.all() and (n_t == k).all() for k, n_t, act in flat)


def test_gpu_clj_calls_render_multi_adaptive():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "render-multi-adaptive" in by_name
    entry = by_name["render-multi-adaptive"]
    called = {x[2].strip('"') for x in walk(entry) if is_list(x, "call-int")}
    assert {"rtmi_init", "rtmi_scene_clone", "rtmi_render_multi_adaptive", "rtmi_adaptive_status", "rtmi_scene_destroy", "rtmi_shutdown"} <= called
    assert "create-scene!" in {x[1] for x in walk(entry) if is_list(x)}
    # the conformance reader accepts the binding: declared symbols, declared arity, coerced scalars, typed arrays, a Pointer array of handles
    flat = [f for f in forms if is_list(f, "defn") and f[2] == "flatten-scene"][0]
    maps = [f for f in walk(flat) if isinstance(f, list) and f[0] == "{" and any(x == ":prim-kind" for x in f[1:])]
    assert check_calls([entry], header_prototypes(), map_values(maps[0]), True, "gpu.clj") >= 5
