"""CPU tests of temporal accumulation's plumbing (rtmi_reproject*): the C-ABI declares, binds and exports both entries, every argument error is
answered without a device by both forms, the Clojure host calls rtmi_reproject, and the CLI checks --accumulate before any device work."""
import ctypes
import os

import numpy as np
import pytest

from raytrace_clj_amd import _ffi
from raytrace_clj_amd import core
from test_clj_conformance import GPU_CLJ, header_prototypes, is_list, read_forms, walk

RTMI_E_ARG, RTMI_E_UNSUPPORTED, RTMI_E_STATE = -1, -3, -5
NAMES = ("rtmi_reproject", "rtmi_reproject_device")
INF, NAN = float("inf"), float("nan")


def test_prototypes_parse_and_match_the_binding():
    protos = header_prototypes()
    head = ["handle", "i32", "i32", "i32", "double[]", "i32", "double[]"]
    scalars = ["f64"] * 5
    assert protos["rtmi_reproject"] == head + ["double[]"] * 7 + scalars + ["double[]", "byte[]", "double[]", "double[]", "long[]"]
    assert protos["rtmi_reproject_device"] == head + ["device-pointer"] * 7 + scalars + ["device-pointer"] * 6
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
    assert L.rtmi_version() >= 211


class _Args:
    """a well-formed call on 8x8 host arrays; fields are replaced per case.  With a NULL handle a well-formed call gets as far as RTMI_E_STATE."""

    def __init__(self):
        z = lambda *s: np.zeros(s)
        self.nx = self.ny = 8
        self.prev_kind, self.prev_cam, self.cur_kind, self.cur_cam = 0, z(24), 1, z(24)
        self.prev_linear, self.prev_weight, self.prev_stderr, self.prev_features = z(8, 8, 3), z(8, 8), z(8, 8), z(8, 8, 8)
        self.cur_linear, self.cur_stderr, self.cur_features = z(8, 8, 3), z(8, 8), z(8, 8, 8)
        self.cur_weight, self.max_history, self.sigma_d, self.sigma_n, self.sigma_a = 4.0, INF, 0.05, 0.0, 0.5
        self.out_linear, self.out_rgb8, self.out_weight, self.out_stderr = z(8, 8, 3), np.zeros((8, 8, 3), np.uint8), z(8, 8), z(8, 8)
        self.out_counters = np.zeros(2, np.uint64)

    def call(self, L, device):
        p = _ffi.ptr
        a = [None, self.nx, self.ny, self.prev_kind, p(self.prev_cam), self.cur_kind, p(self.cur_cam), p(self.prev_linear), p(self.prev_weight),
             p(self.prev_stderr), p(self.prev_features), p(self.cur_linear), p(self.cur_stderr), p(self.cur_features), self.cur_weight,
             self.max_history, self.sigma_d, self.sigma_n, self.sigma_a, p(self.out_linear), p(self.out_rgb8), p(self.out_weight),
             p(self.out_stderr), p(self.out_counters)]
        return L.rtmi_reproject_device(*(a + [None])) if device else L.rtmi_reproject(*a)


def _with(**kw):
    a = _Args()
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_reproject_refuses_bad_arguments_without_a_device(device):
    """every error of the header is decided before the context handle is looked at: with a NULL handle a bad argument is still reported as such,
    and only a well-formed call gets as far as RTMI_E_STATE"""
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    for nx, ny in ((0, 8), (8, 0), (-3, 8), (8, -1)):
        assert _with(nx=nx, ny=ny).call(L, device) == RTMI_E_ARG and "nx" in err()
    for name in ("prev_cam", "cur_cam", "prev_linear", "prev_weight", "prev_features", "cur_linear", "cur_features"):
        assert _with(**{name: None}).call(L, device) == RTMI_E_ARG and name in err(), name
    for bad in (0.0, -1.0, INF, -INF, NAN):
        assert _with(cur_weight=bad).call(L, device) == RTMI_E_ARG and "cur_weight" in err(), bad
    for bad in (0.0, -2.0, -INF, NAN):
        assert _with(max_history=bad).call(L, device) == RTMI_E_ARG and "max_history" in err(), bad
    for k in "dna":
        for bad in (-1.0, -1e-300, NAN, -INF):
            assert _with(**{"sigma_" + k: bad}).call(L, device) == RTMI_E_ARG and "sigma_" + k in err(), (k, bad)
    # out_stderr is written only when both stderr inputs are given
    for name in ("prev_stderr", "cur_stderr"):
        assert _with(**{name: None}).call(L, device) == RTMI_E_ARG and "out_stderr" in err(), name
        assert _with(**{name: None, "out_stderr": None}).call(L, device) == RTMI_E_STATE and "context" in err(), name
    # the history is gathered from neighbours: no output may be a prev_* input
    a = _Args()
    for out, prev in (("out_linear", "prev_linear"), ("out_weight", "prev_weight"), ("out_stderr", "prev_stderr"), ("out_weight", "prev_stderr"),
                      ("out_linear", "prev_features"), ("out_stderr", "prev_weight")):
        assert _with(**{out: getattr(a, prev), prev: getattr(a, prev)}).call(L, device) == RTMI_E_ARG and out in err() and prev in err(), (out, prev)
    # ... but outputs may alias the current frame's buffers
    assert _with(out_linear=a.cur_linear, cur_linear=a.cur_linear, out_stderr=a.cur_stderr, cur_stderr=a.cur_stderr).call(L, device) == RTMI_E_STATE
    # camera kinds
    for name in ("prev_kind", "cur_kind"):
        for bad in (2, -1):
            assert _with(**{name: bad}).call(L, device) == RTMI_E_UNSUPPORTED and "camera kind" in err(), (name, bad)
    # well-formed: every output NULL, max_history +inf, every sigma 0
    assert _Args().call(L, device) == RTMI_E_STATE and "context" in err()
    assert _with(out_linear=None, out_rgb8=None, out_weight=None, out_stderr=None, out_counters=None, sigma_d=0.0, sigma_a=0.0).call(L, device) == RTMI_E_STATE


def test_python_layer_has_the_entry_points():
    for name in ("reproject", "reproject_device"):
        assert callable(getattr(core.Context, name))
    assert callable(core.TemporalAccumulator) and callable(core.TemporalAccumulator.step) and callable(core.TemporalAccumulator.reset)
    assert core.REPROJECT_MAX_HISTORY > 0
    assert min(core.REPROJECT_SIGMA_D, core.REPROJECT_SIGMA_N, core.REPROJECT_SIGMA_A) >= 0


def test_gpu_clj_calls_rtmi_reproject():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "reproject" in by_name
    called = {x[2].strip('"') for x in walk(by_name["reproject"]) if is_list(x, "call-int")}
    assert "rtmi_reproject" in called
    # every scalar of the call is coerced at the call site (test_clj_conformance.py checks the categories against the header)
    call = [x for x in walk(by_name["reproject"]) if is_list(x, "call-int") and x[2] == '"rtmi_reproject"'][0]
    heads = [a[1] if is_list(a) else None for a in call[3:]]
    assert heads.count("int") == 4 and heads.count("double") == 5 and len(call[3:]) == 24


def test_cli_parses_the_accumulate_flag():
    f = core._accumulate_flags
    assert f(["a.png", "8", "8", "4"]) == (["a.png", "8", "8", "4"], None)
    assert f(["a.png", "8", "8", "4", "--accumulate"], 6) == (["a.png", "8", "8", "4"], core.REPROJECT_MAX_HISTORY)
    assert f(["a.png", "--accumulate", "16", "8"], 6) == (["a.png", "8"], 16.0)
    assert f(["--accumulate=inf", "a.png"], 6) == (["a.png"], INF)
    assert f(["--accumulate", "a.png", "--denoise"], 6) == (["a.png", "--denoise"], core.REPROJECT_MAX_HISTORY)
    assert f(["--accumulate", "2.5"], 6) == ([], 2.5)
    assert core._accumulated_name("out/x_003.png") == "out/x_003.acc.png"
    assert core._denoised_name(core._accumulated_name(core._orbit_name("x.ppm", 7))) == "x_007.acc.denoised.ppm"


@pytest.mark.parametrize("flags", [["--accumulate"], ["--accumulate", "16"], ["--orbit", "4", "--accumulate", "0"], ["--orbit", "4", "--accumulate", "-3"],
                                   ["--orbit", "4", "--accumulate=nan"], ["--orbit", "4", "--accumulate=abc"], ["--orbit=4", "--accumulate=-inf"],
                                   ["--orbit", "0", "--accumulate"], ["--orbit", "4", "--accumulate", "--chunk", "4"],
                                   ["--orbit", "4", "--accumulate", "--adaptive", "0.1"], ["--orbit", "4", "--accumulate", "--denoise", "9"],
                                   ["--accumulate", "--chunk", "4"]])
def test_cli_rejects_bad_accumulate_flags_before_device_work(tmp_path, monkeypatch, flags):
    touched = []
    monkeypatch.setattr(core, "DeviceScene", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(core, "TemporalAccumulator", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(core, "render", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(_ffi, "lib", lambda: touched.append(1))
    out = tmp_path / "x.ppm"
    with pytest.raises(SystemExit):
        core.main([str(out), "8", "8", "4"] + flags)
    assert not touched and not list(tmp_path.iterdir())


def test_cli_hands_the_orbit_to_one_accumulator(tmp_path, monkeypatch):
    """--orbit N --accumulate M: one device scene, one accumulator with the cap and the denoise passes as given, one step per view"""
    seen = []

    class FakeScene:
        def __init__(self, *a, **k):
            self.ctx = self

        def progressive_release(self):
            pass

        def close(self):
            pass

    class Stop(Exception):
        pass

    class FakeAccumulator:
        def __init__(self, ds, nx, ny, ns, **kw):
            seen.append((nx, ny, ns, kw))

        def step(self, camera):
            raise Stop

    monkeypatch.setattr(core, "DeviceScene", FakeScene)
    monkeypatch.setattr(core, "TemporalAccumulator", FakeAccumulator)
    for flags, want in ((["--orbit", "3", "--accumulate"], dict(na=core.FEATURE_SAMPLES, max_history=core.REPROJECT_MAX_HISTORY, denoise=None)),
                        (["--accumulate=8", "--orbit=5", "--denoise", "2", "--feature-samples", "1"], dict(na=1, max_history=8.0, denoise={"iterations": 2})),
                        (["--orbit", "2", "--accumulate", "inf"], dict(na=core.FEATURE_SAMPLES, max_history=INF, denoise=None))):
        with pytest.raises(Stop):
            core.main([str(tmp_path / "x.ppm"), "8", "8", "4", "two-spheres"] + flags)
        assert seen[-1] == (8, 8, 4, want), flags
