"""CPU tests of light-sampled frames on several devices (rtmi_lit_tiles_records_device, rtmi_multi_lit_*): the C-ABI declares, binds and exports them, the
argument errors that need no device answer without one, the numpy restatement's dealing, padding and assembly agree with dist.py's and with the dealt
progressive frames' helper, the Clojure host calls the new entries, and the command line refuses --devices without --lit."""
import ctypes
import os

import numpy as np
import pytest

import multi_lit_reference as ml
import multi_progressive_reference as mp
from raytrace_clj_amd import _ffi
from raytrace_clj_amd import core
from raytrace_clj_amd import dist
from test_clj_conformance import GPU_CLJ, check_calls, header_prototypes, is_list, map_values, read_forms, walk

E_ARG, E_STATE = -1, -5
NAMES = ("rtmi_lit_tiles_records_device", "rtmi_multi_lit_create", "rtmi_multi_lit_destroy", "rtmi_multi_lit_render", "rtmi_multi_lit_render_device",
         "rtmi_multi_lit_retire", "rtmi_multi_lit_retire_device", "rtmi_multi_lit_status", "rtmi_multi_lit_active_tiles", "rtmi_multi_lit_reset")
HEADER = os.path.join(os.path.dirname(GPU_CLJ), "..", "..", "..", "include", "rtmi.h")


def test_prototypes_parse_with_the_types_the_reader_knows():
    protos = header_prototypes()
    head = ["i64", "i32", "i32", "i32", "i64", "i32", "i32", "int[]", "i32", "i32"]  # frame precision s_count depth seed estimator n_lights lights choice volume
    assert protos["rtmi_lit_tiles_records_device"] == ["handle"] + ["i32"] * 5 + ["device-pointer"] * 5
    assert protos["rtmi_multi_lit_create"] == ["i32", "handle-array", "i32", "i32", "long[]"]
    assert protos["rtmi_multi_lit_render"] == head + ["double[]", "byte[]", "double[]", "int[]", "long[]"]
    assert protos["rtmi_multi_lit_render_device"] == head + ["device-pointer"] * 5
    assert protos["rtmi_multi_lit_retire"] == ["i64", "double[]", "f64", "int[]"]
    assert protos["rtmi_multi_lit_retire_device"] == ["i64", "device-pointer", "f64", "int[]"]
    assert protos["rtmi_multi_lit_status"] == ["i64", "int[]", "int[]"] and protos["rtmi_multi_lit_active_tiles"] == ["i64", "i32", "int[]", "int[]"]
    assert protos["rtmi_multi_lit_destroy"] == protos["rtmi_multi_lit_reset"] == ["i64"]
    L = _ffi.lib()
    for name in NAMES:
        assert name in _ffi.SYMBOLS and len(getattr(L, name).argtypes) == len(protos[name]), name
    text = open(HEADER).read()
    assert "#define RTMI_MULTI_LIT_MAX 8" in text and ml.MAX_REPLICAS == 8
    assert _ffi.PROG_REC == ml.REC == mp.REC and _ffi.RAYS_REC == ml.RAYS_REC and _ffi.TILE == ml.TILE


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 220


def _render(L, device_form=False, frame=7, precision=0, s_count=2, depth=5, estimator=2, n_lights=0, lights=None, choice=0, volume=0):
    f = L.rtmi_multi_lit_render_device if device_form else L.rtmi_multi_lit_render
    return f(frame, precision, s_count, depth, 1, estimator, n_lights, lights, choice, volume, None, None, None, None, None)


def test_argument_errors_answer_without_a_device():
    """every one of these is RTMI_E_ARG although no frame exists: the arguments are judged before the handle is examined"""
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()  # noqa: E731
    arr, h = (ctypes.c_void_p * 1)(None), ctypes.c_uint64(99)
    for n in (0, -1, 9, 64):
        assert L.rtmi_multi_lit_create(n, arr, 8, 8, ctypes.byref(h)) == E_ARG and "1..8" in err(), n
    assert L.rtmi_multi_lit_create(1, None, 8, 8, ctypes.byref(h)) == E_ARG
    for nx, ny in ((0, 8), (8, 0), (-3, 8), (8, -1)):
        assert L.rtmi_multi_lit_create(1, arr, nx, ny, ctypes.byref(h)) == E_ARG and "nx, ny" in err(), (nx, ny)
    assert L.rtmi_multi_lit_create(1, arr, 8, 8, None) == E_ARG and "out_frame" in err()
    assert L.rtmi_multi_lit_create(1, arr, 8, 8, ctypes.byref(h)) == E_STATE and "scene" in err() and h.value == 99  # a NULL scene: the handle, last
    for device_form in (False, True):
        assert _render(L, device_form, frame=0) == E_ARG and "frame" in err()
        for bad, word in ((dict(s_count=0), "s_count"), (dict(s_count=-4), "s_count"), (dict(depth=-1), "depth"), (dict(estimator=-1), "estimator"),
                          (dict(estimator=4), "estimator"), (dict(volume=2), "volume"), (dict(estimator=3, volume=1), "volume form"),
                          (dict(precision=7), "precision")):
            assert _render(L, device_form, **bad) == E_ARG and word in err(), (device_form, bad, err())
        # what is reported later never hides what is reported first
        assert _render(L, device_form, s_count=0, estimator=9, volume=7, precision=7) == E_ARG and "s_count" in err()
        assert _render(L, device_form, estimator=9, volume=7, precision=7) == E_ARG and "estimator" in err()
        assert _render(L, device_form) == E_STATE and "frame" in err()  # well-formed arguments: the handle names no frame
    n = ctypes.c_int32(-5)
    for f in (L.rtmi_multi_lit_retire, L.rtmi_multi_lit_retire_device):
        assert f(0, None, 0.1, ctypes.byref(n)) == E_ARG and "frame" in err()
        for eps in (-0.5, float("nan"), float("inf")):
            assert f(7, None, eps, ctypes.byref(n)) == E_ARG and "eps" in err(), eps
        assert f(7, None, 0.1, None) == E_ARG and "out_count" in err()
        assert f(7, None, 0.1, ctypes.byref(n)) == E_STATE and n.value == -5
    k = ctypes.c_int32(0)
    assert L.rtmi_multi_lit_status(0, ctypes.byref(k), ctypes.byref(n)) == E_ARG and L.rtmi_multi_lit_status(7, ctypes.byref(k), ctypes.byref(n)) == E_STATE
    assert L.rtmi_multi_lit_reset(0) == E_ARG and L.rtmi_multi_lit_reset(7) == E_STATE
    assert L.rtmi_multi_lit_destroy(0) == E_ARG and L.rtmi_multi_lit_destroy(7) == E_STATE
    assert L.rtmi_multi_lit_active_tiles(0, 4, None, ctypes.byref(n)) == E_ARG and "frame" in err()
    assert L.rtmi_multi_lit_active_tiles(7, -1, None, ctypes.byref(n)) == E_ARG and L.rtmi_multi_lit_active_tiles(7, 4, None, ctypes.byref(n)) == E_ARG
    assert L.rtmi_multi_lit_active_tiles(7, 0, None, None) == E_ARG and L.rtmi_multi_lit_active_tiles(7, 0, None, ctypes.byref(n)) == E_STATE
    # the primitive: the arguments, then the context
    rec = lambda **kw: L.rtmi_lit_tiles_records_device(None, kw.get("nx", 8), kw.get("ny", 8), kw.get("first", 0), kw.get("stride", 1), kw.get("slots", 0),  # noqa: E731
                                                       None, None, None, None, None)
    for bad in (dict(nx=0), dict(ny=-2), dict(first=-1), dict(stride=0), dict(stride=-2), dict(slots=-1), dict(slots=1)):
        assert rec(**bad) == E_ARG and err(), bad
    assert rec() == E_STATE and "context" in err()


@pytest.mark.parametrize("n", ml.WORLDS + (4,))
@pytest.mark.parametrize("size", [ml.SIZE, ml.SMALL, (1920, 1080)])
def test_reference_dealing_and_padding_match_dist(size, n):
    nx, ny = size
    assert ml.n_tiles(nx, ny) == dist.n_tiles(nx, ny) == mp.n_tiles(nx, ny)
    assert ml.per_replica(nx, ny, n) == dist.tiles_per_rank(nx, ny, n) == mp.per_rank(nx, ny, n)
    assert ml.record_words(nx, ny, n) == dist.tiles_per_rank(nx, ny, n) * 320 + 4
    seen = []
    for r in range(n):
        assert ml.owned(nx, ny, r, n) == dist.local_tile_ids(nx, ny, r, n) == mp.local_tiles(nx, ny, r, n)
        assert len(ml.owned(nx, ny, r, n)) <= ml.per_replica(nx, ny, n)
        seen.append(ml.owned(nx, ny, r, n))
    assert ml.merged(seen).tolist() == list(range(ml.n_tiles(nx, ny)))
    if size == ml.SMALL and n == 8:
        assert [len(s) for s in seen] == [1, 1, 1, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("n", ml.WORLDS)
@pytest.mark.parametrize("size", [ml.SIZE, ml.SMALL])
def test_reference_records_and_assembly_against_the_progressive_helper(size, n):
    """hand-made whole-frame buffers: the record read out of them is the dealt progressive frames' record of the same planes, slot by slot, the padding
    and the outside pixels are zeros, and both helpers assemble the gathered records to the planes the records came from"""
    nx, ny = size
    rng = np.random.default_rng(n)
    linear, stderr = rng.random((ny, nx, 3)) + 0.25, rng.random((ny, nx)) + 0.25
    stderr[3, 5], linear[2, 2, 1] = np.inf, 7.5  # a one-sample pixel's error; a mean the quantiser clamps
    samples = rng.integers(1, 9, (ny, nx)).astype(np.int32)
    state = rng.random((nx * ny, ml.RAYS_REC)) - 3.0  # words 0-8 are not the record's business
    state[:, 9] = samples.ravel()
    g = ml.gathered(state, linear, stderr, nx, ny, n)
    per = ml.per_replica(nx, ny, n)
    assert g.shape == (n, per, 64, 5) and g.size == n * (ml.record_words(nx, ny, n) - 4)
    assert np.array_equal(g, mp.gathered_records(linear, stderr, samples, n))
    for r in range(n):
        own = len(ml.owned(nx, ny, r, n))
        assert np.array_equal(g[r, :own], mp.dealt_records(linear, stderr, samples, r, n)) and (g[r, own:] == 0).all()
    got, exp = ml.assemble(g, nx, ny), mp.assemble(g, nx, ny)
    for a, b, c in zip(got, exp, (linear, None, stderr, samples)):
        assert a.dtype == b.dtype and np.array_equal(a, b) and (c is None or np.array_equal(a, c))
    assert got[1][2, 2, 1] == 255 and got[3].dtype == np.int32
    covered = np.zeros((n, per, 64), bool)
    tx = ml.tiles_xy(nx, ny)[0]
    for y in range(ny):
        for x in range(nx):
            t = (y // 8) * tx + x // 8
            covered[t % n, t // n, (y % 8) * 8 + x % 8] = True
    assert covered.sum() == nx * ny and (g[~covered] == 0).all() and (g[covered][:, 4] >= 1).all()


def test_reference_retirement_and_merge():
    nx, ny = ml.SIZE
    noise = np.full((ny, nx), 0.5)
    noise[0:8, 8:16] = 0.01           # tile 1 passes
    noise[16:21, 32:37] = 0.01        # tile 14, partial on both edges, passes on the pixels it has
    noise[8:16, 0:8] = 0.01
    noise[9, 3] = np.nan              # tile 5: a NaN fails
    every = list(range(15))
    assert ml.survivors(noise, 0.1, every, nx, ny) == [t for t in every if t not in (1, 14)]
    assert ml.survivors(noise, 0.1, [14, 1, 5], nx, ny) == [5]  # the order of the list is kept
    lists = [ml.survivors(noise, 0.1, ml.owned(nx, ny, r, 3), nx, ny) for r in range(3)]
    assert ml.merged(lists).tolist() == ml.survivors(noise, 0.1, every, nx, ny)


def test_gpu_clj_calls_the_multi_lit_entries():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "render-multi-lit" in by_name and "render-multi-lit-adaptive" in by_name
    flat = [f for f in forms if is_list(f, "defn") and f[2] == "flatten-scene"][0]
    maps = [f for f in walk(flat) if isinstance(f, list) and f[0] == "{" and any(x == ":prim-kind" for x in f[1:])]
    called = set()
    for name in ("render-multi-lit", "render-multi-lit-adaptive"):
        entry = by_name[name]
        called |= {x[2].strip('"') for x in walk(entry) if is_list(x, "call-int")}
        assert "create-scene!" in {x[1] for x in walk(entry) if is_list(x)}, name
        assert check_calls([entry], header_prototypes(), map_values(maps[0]), True, "gpu.clj") >= 5
    assert {"rtmi_init", "rtmi_scene_clone", "rtmi_multi_lit_create", "rtmi_multi_lit_render", "rtmi_multi_lit_retire", "rtmi_multi_lit_status",
            "rtmi_multi_lit_destroy", "rtmi_scene_destroy", "rtmi_shutdown"} <= called


@pytest.mark.parametrize("argv, word", [
    (["x.ppm", "16", "8", "2", "--devices", "0,0"], "--lit"),
    (["x.ppm", "16", "8", "2", "--devices", "0", "--adaptive", "0.1"], "--lit"),
    (["x.ppm", "16", "8", "2", "--lit", "--devices"], "ordinals"),
    (["x.ppm", "16", "8", "2", "--lit", "--devices", "0,x"], "ordinals"),
    (["x.ppm", "16", "8", "2", "--lit", "--devices=0,1"], "separate word"),
    (["x.ppm", "16", "8", "2", "--lit", "--devices", "0", "--devices", "0"], "twice"),
    (["x.ppm", "16", "8", "2", "--lit-vol", "--devices", "0,0,0,0,0,0,0,0,0"], "at most 8"),
])
def test_cli_refuses_devices_without_a_lit_frame(argv, word):
    """all of them before any device work: no scene is built, nothing is rendered"""
    with pytest.raises(SystemExit) as e:
        core.main(argv)
    assert word in str(e.value), e.value


def test_cli_devices_parser_accepts_what_it_should():
    assert core._devices_flags(["a", "--devices", "0,1,1", "b"], lit=True) == (["a", "b"], [0, 1, 1])
    assert core._devices_flags(["a", "b"], lit=False) == (["a", "b"], None)
