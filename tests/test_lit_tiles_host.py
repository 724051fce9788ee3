"""rtmi_render_lit_tiles* and rtmi_tiles_retire*, the parts that need no GPU: the four prototypes in the header, the Python binding and the Clojure
host; the argument errors that are reported before the handle is examined, in the header's order; and the numpy restatement of THE TILE ORDER and of
the retire rule (tests/lit_tiles_reference.py) against adaptive_reference's tile maxima and against its own definition."""
import ctypes
import os
import re

import numpy as np
import pytest

import adaptive_reference as ar
import lit_tiles_reference as ltr
from raytrace_clj_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtmi_render_lit_tiles", "rtmi_render_lit_tiles_device", "rtmi_tiles_retire", "rtmi_tiles_retire_device")
E_ARG, E_STATE = -1, -5


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(rtmi_(?:render_lit|tiles_retire)\w*)\s*\(([^)]*)\)\s*;", text)}


def test_header_binding_and_clojure_host_declare_the_entries():
    protos = _prototypes()
    assert set(ENTRIES) <= set(protos)
    lit = protos["rtmi_render_lit"]
    tiles = protos["rtmi_render_lit_tiles"]
    k = tiles.index("int32_t volume")
    assert tiles[:k] + tiles[k + 3:] == lit and tiles[k:k + 3] == ["int32_t volume", "int32_t n_tiles", "const int32_t *tiles"]
    dev = protos["rtmi_render_lit_tiles_device"]
    assert dev[:k] + dev[k + 3:] == protos["rtmi_render_lit_device"] and dev[k + 2].replace(" ", "") == "constvoid*d_tiles"
    assert len(protos["rtmi_tiles_retire"]) == 9 and len(protos["rtmi_tiles_retire_device"]) == 10
    L = _ffi.lib()
    for name in ENTRIES:
        assert name in _ffi.SYMBOLS and len(getattr(L, name).argtypes) == len(protos[name]), name
        if name.endswith("_device"):
            assert protos[name][-1].replace(" ", "") == "void*stream" and len(protos[name]) == len(protos[name[:-7]]) + 1
    assert L.rtmi_version() >= 219
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "THE TILE ORDER" in header
    clj = open(os.path.join(ROOT, "clj", "src", "raytrace_clj", "gpu.clj")).read()
    for fn, sym in (("render-lit-tiles", "rtmi_render_lit_tiles"), ("tiles-retire", "rtmi_tiles_retire"), ("render-lit-adaptive", "rtmi_render_lit_tiles")):
        body = clj.split("(defn %s\n" % fn, 1)
        assert len(body) == 2, fn
        assert '(call-int "%s" ' % sym in body[1].split("\n(defn ", 1)[0], fn


def test_argument_errors_come_before_the_handle_in_the_headers_order():
    L, p = _ffi.lib(), _ffi.ptr
    err = lambda: L.rtmi_last_error().decode()  # noqa: E731
    nx, ny = 13, 7
    lin, se, tiles = np.zeros((ny, nx, 3)), np.zeros((ny, nx)), np.array([0, 1], np.int32)
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)

    def host(nx=nx, ny=ny, s_first=0, s_count=1, depth=5, estimator=2, volume=0, n_tiles=2, tl=tiles, out=lin, n_lights=0, prims=None):
        return L.rtmi_render_lit_tiles(None, 0, nx, ny, s_first, s_count, depth, 1, estimator, n_lights, p(prims), 0, volume, n_tiles, p(tl), None, p(out), None,
                                       p(se), None, None, None)

    def device(nx=nx, ny=ny, s_first=0, s_count=1, depth=5, estimator=2, volume=0, n_tiles=2, tl=tiles, out=lin, n_lights=0, prims=None):
        return L.rtmi_render_lit_tiles_device(None, 0, nx, ny, s_first, s_count, depth, 1, estimator, n_lights, p(prims), 0, volume, n_tiles, p(tl), None, p(out),
                                              None, p(se), None, None, None, None)
    bad = np.array([0, 2], np.int32)  # 13 x 7 has two tiles
    for f in (host, device):
        late = dict(estimator=9, volume=7, n_tiles=-1, out=None)  # what is reported later never hides what is reported first
        assert f(nx=0, **late) == E_ARG and "s_count" in err()
        assert f(s_count=0, **late) == E_ARG and f(s_first=-1, **late) == E_ARG and f(depth=-1, **late) == E_ARG
        assert f(s_count=1 << 20, **dict(late, n_tiles=1 << 20)) == E_ARG and "2^31 - 64" in err()   # the limit is on n_tiles * 64 * s_count ...
        assert f(nx=1 << 16, ny=1 << 16, **late) == E_ARG and "2^31 - 64" in err()
        assert f(s_first=(1 << 31) - 1, **late) == E_ARG and "overflows" in err()
        assert f(**late) == E_ARG and "NULL" in err()
        assert f(**dict(late, out=lin)) == E_ARG and "estimator" in err()
        assert f(volume=7, n_tiles=-1) == E_ARG and "volume" in err()
        assert f(volume=-1) == E_ARG and f(volume=2) == E_ARG
        assert f(n_tiles=-1, tl=bad) == E_ARG and "n_tiles" in err()
        assert f(n_tiles=2, tl=None) == E_ARG and "n_tiles" in err()
        # ... not on the frame: 4096 x 4096 x 256 is refused by rtmi_render_lit and taken here with two tiles listed
        assert f(nx=4096, ny=4096, s_count=256, out=lin) == E_STATE
        assert f(n_lights=len(many), prims=many) == E_STATE  # sound arguments: the NULL handle is what is wrong; the lights come behind it
        assert f(n_tiles=0, tl=None) == E_STATE              # an empty list passes the argument checks
    # the list's entries: the host form alone reads them
    assert host(tl=bad) == E_ARG and "tiles[1] = 2" in err() and device(tl=bad) == E_STATE
    assert host(tl=np.array([-1, 0], np.int32)) == E_ARG and "tiles[0]" in err()
    assert host(tl=np.array([1, 1], np.int32)) == E_ARG and "ascending" in err()
    assert host(tl=np.array([1, 0], np.int32)) == E_ARG and "ascending" in err()
    assert host(volume=1, tl=bad) == E_ARG and "tiles[1]" in err()

    noise, out, n = np.zeros((ny, nx)), np.zeros(2, np.int32), ctypes.c_int32(-3)
    rt = lambda nx=nx, ny=ny, m=noise, eps=0.5, nt=2, tin=tiles, tout=out, cnt=ctypes.byref(n): \
        L.rtmi_tiles_retire(None, nx, ny, p(m), eps, nt, p(tin), p(tout), cnt)  # noqa: E731
    rt_d = lambda nx=nx, ny=ny, m=noise, eps=0.5, nt=2, tin=tiles, tout=out, cnt=ctypes.byref(n): \
        L.rtmi_tiles_retire_device(None, nx, ny, p(m), eps, nt, p(tin), p(tout), cnt, None)  # noqa: E731
    for f in (rt, rt_d):
        assert f(nx=0, m=None, eps=-1.0, nt=-1) == E_ARG and "nx, ny" in err()
        assert f(ny=-2) == E_ARG
        assert f(m=None, eps=-1.0, nt=-1) == E_ARG and "noise" in err()
        for eps in (-1e-300, float("nan"), float("inf"), float("-inf")):
            assert f(eps=eps, nt=-1) == E_ARG and "eps" in err()
        assert f(nt=-1) == E_ARG and "n_tiles" in err()
        assert f(tin=None) == E_ARG and f(tout=None) == E_ARG and f(cnt=None) == E_ARG
        assert f() == E_STATE and f(eps=0.0) == E_STATE and f(nt=0, tin=None, tout=None) == E_STATE
    assert rt(tin=bad) == E_ARG and "tiles_in[1]" in err() and rt_d(tin=bad) == E_STATE
    assert n.value == -3 and (out == 0).all()


@pytest.mark.parametrize("shape", ltr.RETIRE_SHAPES)
def test_reference_retire_rule_is_the_tile_maximum_rule(shape):
    nx, ny = shape
    tx, ty = ltr.tiles_of(nx, ny)
    every = ltr.all_tiles(nx, ny)
    seen = set()
    for name, noise, eps in ltr.retire_maps(nx, ny):
        with np.errstate(invalid="ignore"):
            passes = (ar.tile_max(noise) <= eps).reshape(-1)  # a NaN propagates through the maximum and fails
        want = every[~passes]
        assert np.array_equal(ltr.retire(noise, eps, every), want), name
        sub = every[::2]
        assert np.array_equal(ltr.retire(noise, eps, sub), sub[~passes[::2]]), name
        assert np.array_equal(ltr.retire(noise, eps, every[::-1]), want[::-1]), name  # the order is the list's
        seen.add((name, len(want)))
    got = dict(seen)
    n = tx * ty
    assert got["ties-all-pass"] == 0 and got["ties-one-ulp"] == (n + 1) // 2 and got["all -inf"] == 0 and got["-inf"] == 0
    assert got["nan"] == (2 if n > 1 else 1) and got["+inf"] == got["nan"] and 0 < got["uniform"]
    assert nx % 8 and ny % 8  # partial tiles on both edges


@pytest.mark.parametrize("shape", ((13, 7, 3), (21, 19, 2)))
def test_reference_row_map_is_a_bijection_onto_listed_pixels_and_samples(shape):
    nx, ny, ns = shape
    every = ltr.all_tiles(nx, ny)
    for tiles, s_first in ((every, 0), (every[every % 3 != 1], 4), (every[-1:], 1)):
        x, y, s, has = ltr.row_map(nx, ny, s_first, ns, tiles)
        assert len(has) == len(tiles) * 64 * ns
        mask = ltr.pixel_mask(nx, ny, tiles)
        got = sorted(zip(x[has].tolist(), y[has].tolist(), s[has].tolist()))
        want = sorted((int(px), int(py), s_first + k) for py, px in zip(*np.nonzero(mask)) for k in range(ns))
        assert got == want and len(set(got)) == len(got) == int(mask.sum()) * ns
        assert (x[~has] == 0).all() and (y[~has] == 0).all() and (s[~has] == 0).all() and (~has).any()
        # a tile's rows are consecutive, a pixel's samples innermost, the local pixel row-major in the tile
        r = np.arange(len(has))
        tx = ltr.tiles_of(nx, ny)[0]
        assert np.array_equal((y[has] // 8) * tx + x[has] // 8, np.asarray(tiles)[r[has] // (64 * ns)])
        assert np.array_equal((y[has] % 8) * 8 + x[has] % 8, (r[has] // ns) % 64) and np.array_equal(s[has] - s_first, r[has] % ns)
    # with every tile listed the map reaches every row of the frame call exactly once
    has, rows = ltr.frame_rows(nx, ny, 0, ns, every)
    assert np.array_equal(np.sort(rows), np.arange(nx * ny * ns))
    # entries outside [0, T) hold no pixel
    x, y, s, has = ltr.row_map(nx, ny, 0, ns, [-1, 0, len(every), 2 ** 31 - 1])
    assert not has[:64 * ns].any() and not has[2 * 64 * ns:].any() and has[64 * ns:2 * 64 * ns].any()
