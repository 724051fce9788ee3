"""CPU tests of adaptive sampling (rtmi_render_adaptive*, rtmi_adaptive_status): the C-ABI declares, binds and exports it, its handle checks
answer without a device, the Clojure host calls it, and the CLI checks --adaptive before any device work."""
import ctypes
import os

import pytest

from raytrace_clj_amd import _ffi
from raytrace_clj_amd import core
from test_clj_conformance import GPU_CLJ, header_prototypes, is_list, read_forms, walk

RTMI_E_STATE = -5
NAMES = ("rtmi_render_adaptive", "rtmi_render_adaptive_device", "rtmi_adaptive_status", "rtmi_adaptive_active_tiles")


def test_adaptive_prototypes_parse():
    protos = header_prototypes()
    assert protos["rtmi_render_adaptive"] == ["handle", "i32", "i32", "i32", "i32", "f64", "i32", "i64", "i32", "i32", "i32", "i32", "i32",
                                              "double[]", "byte[]", "double[]", "int[]", "long[]"]
    assert protos["rtmi_render_adaptive_device"] == ["handle", "i32", "i32", "i32", "i32", "f64", "i32", "i64", "i32"] + ["device-pointer"] * 6
    assert protos["rtmi_adaptive_status"] == ["handle", "int[]", "int[]", "long[]"]
    assert protos["rtmi_adaptive_active_tiles"] == ["handle", "i32", "int[]", "int[]"]
    assert set(NAMES) <= set(_ffi.SYMBOLS)


def test_library_exports_adaptive_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 206


def test_adaptive_entries_reject_null_handles_without_a_device():
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    assert L.rtmi_render_adaptive(None, 8, 8, 0, 2, 0.1, 50, 1, 0, 0, 0, 8, 8, None, None, None, None, None) == RTMI_E_STATE and err()
    assert L.rtmi_render_adaptive_device(None, 8, 8, 0, 2, 0.1, 50, 1, 0, None, None, None, None, None, None) == RTMI_E_STATE and err()
    a, t, n = ctypes.c_int32(7), ctypes.c_int32(8), ctypes.c_int64(9)
    assert L.rtmi_adaptive_status(None, ctypes.byref(a), ctypes.byref(t), ctypes.byref(n)) == RTMI_E_STATE and "context" in err()
    assert (a.value, t.value, n.value) == (7, 8, 9)
    assert L.rtmi_adaptive_active_tiles(None, 0, None, ctypes.byref(a)) == RTMI_E_STATE and "context" in err() and a.value == 7


def test_gpu_clj_calls_render_adaptive():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "render-adaptive" in by_name
    called = {x[2].strip('"') for x in walk(by_name["render-adaptive"]) if is_list(x, "call-int")}
    assert {"rtmi_render_adaptive", "rtmi_adaptive_status"} <= called
    assert "create-scene!" in {x[1] for x in walk(by_name["render-adaptive"]) if is_list(x)}


@pytest.mark.parametrize("flags", [["--adaptive", "-1"], ["--adaptive", "nan"], ["--adaptive", "abc"], ["--adaptive"], ["--adaptive", "inf"],
                                   ["--adaptive", "0.1", "--noise", "0.1"], ["--noise=0.1", "--adaptive=0.1"],
                                   ["--adaptive", "0.1", "--chunk", "0"]])
def test_cli_rejects_bad_adaptive_flags_before_device_work(tmp_path, monkeypatch, flags):
    touched = []
    monkeypatch.setattr(core, "DeviceScene", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(core, "render", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(_ffi, "lib", lambda: touched.append(1))
    out = tmp_path / "x.ppm"
    with pytest.raises(SystemExit):
        core.main([str(out), "8", "8", "4"] + flags)
    assert not touched and not out.exists()
