"""CPU tests of the feature pass and the denoiser (rtmi_render_features*, rtmi_denoise*): the C-ABI declares, binds and exports them, their
argument checks answer without a device, the Clojure host calls them, and the CLI checks --denoise / --feature-samples before any device work."""
import ctypes
import os

import numpy as np
import pytest

from raytrace_clj_amd import _ffi
from raytrace_clj_amd import core
from test_clj_conformance import GPU_CLJ, header_prototypes, is_list, read_forms, walk

RTMI_E_ARG, RTMI_E_STATE = -1, -5
NAMES = ("rtmi_render_features", "rtmi_render_features_device", "rtmi_denoise", "rtmi_denoise_device")


def test_prototypes_parse_and_match_the_binding():
    protos = header_prototypes()
    assert protos["rtmi_render_features"] == ["handle", "i32", "i32", "i32", "i64", "i32", "i32", "i32", "i32", "i32", "double[]", "long[]"]
    assert protos["rtmi_render_features_device"] == ["handle", "i32", "i32", "i32", "i64", "i32"] + ["device-pointer"] * 3
    assert protos["rtmi_denoise"] == ["handle", "i32", "i32", "double[]", "double[]", "double[]", "i32", "f64", "f64", "f64", "f64",
                                      "double[]", "byte[]", "double[]"]
    assert protos["rtmi_denoise_device"] == ["handle", "i32", "i32"] + ["device-pointer"] * 3 + ["i32", "f64", "f64", "f64", "f64"] + ["device-pointer"] * 4
    assert set(NAMES) <= set(_ffi.SYMBOLS)
    assert sorted(protos) == sorted(_ffi.SYMBOLS)
    L = _ffi.lib()
    for name in NAMES:  # the bound argument lists have the header's lengths
        assert len(getattr(L, name).argtypes) == len(protos[name]), name


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 207


def _denoise(L, device, nx=8, ny=8, lin=True, iterations=1, sigmas=(1.0, 1.0, 1.0, 1.0)):
    buf = np.zeros((8, 8, 3))
    args = [None, nx, ny, _ffi.ptr(buf) if lin else None, None, None, iterations] + list(sigmas) + [None, None, None]
    return L.rtmi_denoise_device(*(args + [None])) if device else L.rtmi_denoise(*args)


@pytest.mark.parametrize("device", [False, True])
def test_denoise_refuses_bad_arguments_without_a_device(device):
    """every RTMI_E_ARG case is decided before the context handle is looked at: with a NULL handle a bad argument is still RTMI_E_ARG, and only a
    well-formed call gets as far as RTMI_E_STATE"""
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    for it in (-1, 9, 100):
        assert _denoise(L, device, iterations=it) == RTMI_E_ARG and "iterations" in err()
    for k in range(4):
        for bad in (-1.0, -1e-300, float("nan"), float("-inf")):
            sg = [1.0] * 4
            sg[k] = bad
            assert _denoise(L, device, sigmas=sg) == RTMI_E_ARG and "sigma_" + "cnad"[k] in err(), (k, bad)
    for nx, ny in ((0, 8), (8, 0), (-3, 8), (8, -1)):
        assert _denoise(L, device, nx=nx, ny=ny) == RTMI_E_ARG and "nx" in err()
    assert _denoise(L, device, lin=False) == RTMI_E_ARG and "linear_in" in err()
    for it in (0, 8):
        assert _denoise(L, device, iterations=it, sigmas=(0.0, 0.0, 0.0, float("inf"))) == RTMI_E_STATE and "context" in err()


def test_features_refuse_bad_arguments_without_a_device():
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    for na in (0, -1):
        assert L.rtmi_render_features(None, 8, 8, na, 1, 0, 0, 0, 8, 8, None, None) == RTMI_E_ARG and "na" in err()
        assert L.rtmi_render_features_device(None, 8, 8, na, 1, 0, None, None, None) == RTMI_E_ARG and "na" in err()
    assert L.rtmi_render_features(None, 0, 8, 1, 1, 0, 0, 0, 8, 8, None, None) == RTMI_E_ARG
    assert L.rtmi_render_features(None, 8, 8, 1, 1, 0, 0, 0, 8, 8, None, None) == RTMI_E_STATE and "scene" in err()
    assert L.rtmi_render_features_device(None, 8, 8, 1, 1, 0, None, None, None) == RTMI_E_STATE and "scene" in err()


def test_python_layer_has_the_entry_points():
    for name in ("render_features", "render_features_device", "render_denoised"):
        assert callable(getattr(core.DeviceScene, name))
    for name in ("denoise", "denoise_device"):
        assert callable(getattr(core.Context, name))
    assert 0 <= core.DENOISE_ITERATIONS <= 8 and core.FEATURE_SAMPLES > 0
    assert min(core.DENOISE_SIGMA_C, core.DENOISE_SIGMA_N, core.DENOISE_SIGMA_A, core.DENOISE_SIGMA_D) >= 0


def test_gpu_clj_calls_the_entries():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "render-features" in by_name and "denoise" in by_name
    called = {x[2].strip('"') for x in walk(by_name["render-features"]) if is_list(x, "call-int")}
    assert "rtmi_render_features" in called
    assert "create-scene!" in {x[1] for x in walk(by_name["render-features"]) if is_list(x)}
    called = {x[2].strip('"') for x in walk(by_name["denoise"]) if is_list(x, "call-int")}
    assert "rtmi_denoise" in called


def test_cli_parses_the_denoise_flags():
    f = core._denoise_flags
    assert f(["a.png", "8", "8", "4"]) == (["a.png", "8", "8", "4"], None, None)
    assert f(["a.png", "8", "8", "4", "--denoise"]) == (["a.png", "8", "8", "4"], core.DENOISE_ITERATIONS, None)
    assert f(["a.png", "8", "8", "4", "--denoise", "3"]) == (["a.png", "8", "8", "4"], 3, None)
    assert f(["a.png", "8", "8", "4", "--denoise=0", "--feature-samples", "2"]) == (["a.png", "8", "8", "4"], 0, 2)
    assert f(["--denoise", "a.png", "8", "8", "4", "--feature-samples=16", "--chunk", "4"]) == (["a.png", "8", "8", "4", "--chunk", "4"], core.DENOISE_ITERATIONS, 16)
    assert f(["a.png", "--denoise", "--adaptive", "0.1"]) == (["a.png", "--adaptive", "0.1"], core.DENOISE_ITERATIONS, None)
    assert core._denoised_name("out/x.png") == "out/x.denoised.png" and core._denoised_name("x.ppm") == "x.denoised.ppm"


@pytest.mark.parametrize("flags", [["--denoise", "9"], ["--denoise", "-1"], ["--denoise=abc"], ["--denoise=2.5"], ["--feature-samples", "4"],
                                   ["--denoise", "--feature-samples"], ["--denoise", "--feature-samples", "0"],
                                   ["--denoise", "--feature-samples", "-2"], ["--denoise", "--feature-samples", "x"],
                                   ["--denoise", "3", "--chunk", "0"], ["--denoise", "--adaptive", "-1"]])
def test_cli_rejects_bad_denoise_flags_before_device_work(tmp_path, monkeypatch, flags):
    touched = []
    monkeypatch.setattr(core, "DeviceScene", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(core, "render", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(_ffi, "lib", lambda: touched.append(1))
    out = tmp_path / "x.ppm"
    with pytest.raises(SystemExit):
        core.main([str(out), "8", "8", "4"] + flags)
    assert not touched and not out.exists() and not (tmp_path / "x.denoised.ppm").exists()
