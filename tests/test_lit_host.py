"""CPU side of rtmi_render_lit: the entries exist and are declared, the argument errors that stand before the handle check come back in the header's
order, the python and command-line refusals happen before any device work, and the reference chain test_gpu_lit.py compares the device with -- the
frame's samples one by one (lit_cases.frame_groups), the oracle's paths from each sample's own stream position, rays_reference.fold -- is the oracle's
own frame, bit for bit.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

import lit_cases as lc
from raytrace_clj_amd import _ffi, core
from tests import direct_cases as dcs

RTMI_E_ARG, RTMI_E_STATE = -1, -5


def test_the_library_exports_both_entries_and_ffi_declares_them():
    L = _ffi.lib()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("rtmi_render_lit", 19), ("rtmi_render_lit_device", 20)):
        assert name in _ffi.SYMBOLS
        assert getattr(raw, name) is not None
        assert len(getattr(L, name).argtypes) == n_args
    assert core.LIT_ESTIMATORS == lc.ESTIMATORS


@pytest.mark.parametrize("device_form", [False, True])
def test_argument_errors_in_the_headers_order(device_form):
    """with a NULL scene: every error that precedes the handle check, each reached only once the ones before it are mended, then RTMI_E_STATE"""
    L = _ffi.lib()
    lin, se = np.full((2, 2, 3), -7.0), np.full((2, 2), -7.0)
    err = lambda: L.rtmi_last_error().decode()

    def call(nx=2, ny=2, s_first=0, s_count=1, depth=5, estimator=2, out_linear=lin, out_stderr=se, n_lights=0, choice=0, precision=0):
        args = [None, precision, nx, ny, s_first, s_count, depth, 1, estimator, n_lights, None, choice, None, core.ptr(out_linear), None,
                core.ptr(out_stderr), None, None, None]
        return L.rtmi_render_lit_device(*args, None) if device_form else L.rtmi_render_lit(*args)
    bad = dict(estimator=9, out_linear=None, precision=7, n_lights=-1, choice=5)  # what comes later never hides what comes first
    for kw in (dict(nx=0), dict(ny=0), dict(s_count=0), dict(nx=-1), dict(s_first=-1), dict(depth=-1)):
        assert call(**dict(bad, **kw)) == RTMI_E_ARG and "s_count" in err(), kw
    for kw in (dict(nx=1 << 16, ny=1 << 16), dict(nx=1 << 15, ny=1 << 15, s_count=2), dict(nx=1 << 30, ny=1 << 30, s_count=1 << 30),
               dict(nx=1 << 10, ny=1 << 10, s_count=(1 << 11))):
        assert call(**dict(bad, **kw)) == RTMI_E_ARG and "2^31 - 64" in err(), kw
    assert call(**dict(bad, s_first=(1 << 31) - 1, s_count=1)) == RTMI_E_ARG and "overflows" in err()
    assert call(**dict(bad, s_first=(1 << 31) - 2, s_count=1, out_linear=lin)) == RTMI_E_ARG and "estimator" in err()  # (no overflow: the next error)
    assert call(**bad) == RTMI_E_ARG and "NULL" in err()
    assert call(**dict(bad, out_linear=lin, out_stderr=None)) == RTMI_E_ARG and "NULL" in err()
    for e in (-1, 3, 9):
        assert call(**dict(bad, out_linear=lin, estimator=e)) == RTMI_E_ARG and "estimator" in err()
    for e in (0, 1, 2):  # the handle comes before the precision and the lights
        assert call(**dict(bad, out_linear=lin, estimator=e)) == RTMI_E_STATE and "scene" in err()
    assert (lin == -7.0).all() and (se == -7.0).all()


def test_estimator_names_are_refused_before_any_device_work():
    ds = object.__new__(core.DeviceScene)  # no context, no handle: anything past the name check would fail on them
    for name in ("bdpt", "", "MIS", 3, -1, True):
        with pytest.raises(ValueError):
            ds.render_lit(8, 8, 1, estimator=name)
        with pytest.raises(ValueError):
            ds.render_lit_device(8, 8, 0, 1, None, None, estimator=name)
    assert [core.DeviceScene._lit_estimator(n) for n in ("plain", "nee", "mis", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]


def test_lit_flag_parsing_and_refusals(monkeypatch):
    """--lit takes an optional word; what it does not combine with is refused before any device work (DeviceScene is never built)"""
    def no_device(*a, **k):
        raise AssertionError("device work before the flags were checked")
    monkeypatch.setattr(core, "DeviceScene", no_device)
    monkeypatch.setattr(core, "render", no_device)
    assert core._lit_flags(["a.png", "--lit", "8"]) == (["a.png", "8"], ("mis", "uniform"))
    assert core._lit_flags(["a.png", "8", "--lit"]) == (["a.png", "8"], ("mis", "uniform")) and core._lit_flags(["a.png"]) == (["a.png"], None)
    assert core._lit_flags(["--lit", "plain", "a.png"]) == (["a.png"], ("plain", "uniform"))
    assert core._lit_flags(["a.png", "--lit", "nee"]) == (["a.png"], ("nee", "uniform"))
    assert core._lit_flags(["a.png", "--lit", "mis:power", "8"]) == (["a.png", "8"], ("mis", "power"))
    assert core._lit_flags(["a.png", "--lit", "mis:uniform"]) == (["a.png"], ("mis", "uniform"))
    assert core._lit_name("out/a.png") == "out/a.lit.png"
    for argv, word in ((["a.png", "8", "8", "1", "--lit=mis"], "separate word"),
                       (["a.png", "8", "8", "1", "--lit", "--lit"], "twice"),
                       (["a.png", "8", "8", "1", "--lit", "nee:power"], "mis:power"),
                       (["a.png", "8", "8", "1", "--lit", "mis:brightest"], "mis:power"),
                       (["a.png", "8", "8", "1", "--lit", "--panorama"], "--panorama"),
                       (["a.png", "8", "8", "1", "--lit", "mis:power", "--orbit", "4"], "--orbit"),
                       (["a.png", "8", "8", "1", "cornell-box-classic", "--lit", "--nee"], "--nee"),
                       (["a.png", "8", "8", "1", "cornell-box-classic", "--mis", "power", "--lit", "plain"], "--mis"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit"], "ConstantMedium"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit", "nee", "--chunk", "2"], "ConstantMedium")):
        with pytest.raises(SystemExit) as ei:
            core.main(argv)
        assert word in str(ei.value), (argv, ei.value)
    for argv in (["a.png", "8", "8", "1", "cornell-box-classic", "--lit", "mis:power"], ["a.png", "8", "8", "1", "cornell-box", "--lit", "plain"]):
        with pytest.raises(AssertionError):  # a combination it does render gets as far as the device (the plain estimator traces media)
            core.main(argv)


@pytest.mark.parametrize("name", ("sphere-lamp", "cornell"))
def test_the_reference_chain_is_the_oracles_frame(oracle, name):
    """the frame's samples in the call's row order, the oracle's path of each from its own stream position, the restated fold = Oracle.render"""
    nx, ny, ns = lc.SMALL
    f = dcs.flat(name)
    rays, keys, ctr = lc.frame_groups(lambda uv, k: oracle.probe_camera(f, uv, k), f, nx, ny, ns)
    assert np.array_equal(keys, lc.frame_keys(nx, ny, ns)) and len(np.unique(ctr)) > 1  # a thin lens: the paths start at different draws
    rgb, nseg, _, _ = lc.probe_by_ctr(lambda r, k, ctr0: oracle.probe_paths(f, r, k, depth=50, ctr0=ctr0), rays, keys, ctr)
    lin, err = lc.folded_frame(rgb, nx, ny, ns)
    elin, _, cnt = oracle.render(f, nx, ny, ns, 50, lc.SEED)
    assert np.array_equal(lc.bits(lin), lc.bits(elin)), "%d pixels differ" % (lin != elin).any(axis=2).sum()
    assert int(nseg.sum()) == int(cnt[0]) and int(cnt[1]) == nx * ny
    assert np.isfinite(err).all() and (err > 0).any()
    # a chunk of the samples is the same rows of the whole
    part = lc.frame_groups(lambda uv, k: oracle.probe_camera(f, uv, k), f, nx, ny, 2, s_first=1)
    pick = (np.arange(nx * ny)[:, None] * ns + np.arange(1, 3)[None, :]).ravel()
    assert all(np.array_equal(a, b[pick]) for a, b in zip(part, (rays, keys, ctr)))
