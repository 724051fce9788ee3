"""CPU tests of progressive rendering (rtmi_render_progressive*): the C-ABI declares, binds and exports it, its handle checks answer
without a device, the Clojure host calls it, and the CLI checks its flags before any device work."""
import ctypes
import os

import pytest

from raytrace_clj_amd import _ffi
from raytrace_clj_amd import core
from test_clj_conformance import GPU_CLJ, header_prototypes, is_list, read_forms, walk

RTMI_E_STATE = -5
NAMES = ("rtmi_render_progressive", "rtmi_render_progressive_device", "rtmi_progressive_samples", "rtmi_progressive_release")


def test_progressive_prototypes_parse():
    protos = header_prototypes()
    assert protos["rtmi_render_progressive"] == ["handle", "i32", "i32", "i32", "i32", "i32", "i64", "i32", "i32", "i32", "i32", "i32",
                                                 "double[]", "byte[]", "double[]", "long[]"]
    assert protos["rtmi_render_progressive_device"] == ["handle", "i32", "i32", "i32", "i32", "i32", "i64", "i32",
                                                        "device-pointer", "device-pointer", "device-pointer", "device-pointer", "device-pointer"]
    assert protos["rtmi_progressive_samples"] == ["handle", "int[]"]
    assert protos["rtmi_progressive_release"] == ["handle"]
    assert set(NAMES) <= set(_ffi.SYMBOLS)


def test_library_exports_progressive_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 205


def test_progressive_entries_reject_null_handles_without_a_device():
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    assert L.rtmi_render_progressive(None, 8, 8, 0, 1, 50, 1, 0, 0, 0, 8, 8, None, None, None, None) == RTMI_E_STATE and err()
    assert L.rtmi_render_progressive_device(None, 8, 8, 0, 1, 50, 1, 0, None, None, None, None, None) == RTMI_E_STATE and err()
    k = ctypes.c_int32(7)
    assert L.rtmi_progressive_samples(None, ctypes.byref(k)) == RTMI_E_STATE and err() and k.value == 7
    assert L.rtmi_progressive_release(None) == RTMI_E_STATE and "context" in err()


def test_gpu_clj_calls_render_progressive():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "render-progressive" in by_name
    called = {x[2].strip('"') for x in walk(by_name["render-progressive"]) if is_list(x, "call-int")}
    assert "rtmi_render_progressive" in called
    assert "create-scene!" in {x[1] for x in walk(by_name["render-progressive"]) if is_list(x)}


@pytest.mark.parametrize("flags", [["--chunk", "0"], ["--chunk", "-3"], ["--chunk", "two"], ["--budget", "-1"], ["--budget", "nan"],
                                   ["--noise", "abc"], ["--noise", "-1e-3"], ["--chunk"]])
def test_cli_rejects_bad_progressive_flags_before_device_work(tmp_path, monkeypatch, flags):
    touched = []
    monkeypatch.setattr(core, "DeviceScene", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(core, "render", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(_ffi, "lib", lambda: touched.append(1))
    out = tmp_path / "x.ppm"
    with pytest.raises(SystemExit):
        core.main([str(out), "8", "8", "4"] + flags)
    assert not touched and not out.exists()
