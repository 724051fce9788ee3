"""CPU side of adaptive sampling steered by the denoised frame's noise estimate (rtmi_adaptive_retire*, refine_adaptive_denoised):

  * the inputs of test_gpu_adaptive_denoised.py's oracle cases, judged on the CPU oracle and the numpy filter alone -- conditions on the
    inputs, not tolerances: a changed fixture must not make the GPU test vacuous;
  * the retirement rule on hand-made maps through the numpy model (adaptive_denoised_reference.retire), against expectations written per map;
  * the CLI checks --adaptive-denoised before any device work; the header declares, _ffi binds and the built library exports the two entries;
    the Clojure host calls them.

Measured when the cases were chosen (active tiles after every round, of the frame's tiles):

  spheres 61x37  f64 / f32  16 / 16 / 64  eps 0.2    30, 27, 24, 16 of 40
  mixed   61x37  f64        16 / 16 / 64  eps 0.1    28, 26, 24, 24 of 40
  spheres 203x99 f64        8 / 8 / 48    eps 0.15   142, 120, 101, 93, 84, 81 of 338

If a case stops meeting a condition (a scene of frame_reference.py was edited), choose another eps; do not loosen the condition."""
import ctypes
import os

import numpy as np
import pytest

import adaptive_denoised_reference as adr
import adaptive_reference as ar
import frame_reference as fr
from raytrace_clj_amd import _ffi
from raytrace_clj_amd import core
from test_clj_conformance import GPU_CLJ, header_prototypes, is_list, read_forms, walk

RTMI_E_ARG, RTMI_E_STATE = -1, -5
NAMES = ("rtmi_adaptive_retire", "rtmi_adaptive_retire_device")


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


def test_the_model_filters_with_the_library_defaults():
    assert adr.FILTER == dict(iterations=core.DENOISE_ITERATIONS, sigma_c=core.DENOISE_SIGMA_C, sigma_n=core.DENOISE_SIGMA_N,
                              sigma_a=core.DENOISE_SIGMA_A, sigma_d=core.DENOISE_SIGMA_D) and adr.NA == core.FEATURE_SAMPLES
    assert [c[:6] for c in adr.CASES] == [c[:6] for c in ar.CASES], "the scenes, sizes and rounds of the raw-criterion cases"


@pytest.mark.parametrize("case", adr.CASES, ids=ar.case_id)
def test_case_is_fit_to_test_with(request, case):
    name, precision, (nx, ny), first, chunk, cap, eps = case
    o = _oracle(request, precision)
    smp, nseg, feat, rounds = adr.reference_run(o, case)
    last = rounds[-1]
    total = last["active"].size
    schedule = [int(r["active"].sum()) for r in rounds]
    levels, counts = np.unique(last["n_t"], return_counts=True)
    print(ar.case_id(case), "active after every round:", schedule, "of", total, dict(zip(levels.tolist(), counts.tolist())))
    assert last["k"] == cap
    assert len(levels) >= 3, levels
    assert total - schedule[-1] >= total / 5, "at least a fifth of the tiles retired by the end"
    assert schedule[-1] >= total / 5, "at least a fifth of the tiles still active at the cap"
    retired_in = [a - b for a, b in zip([total] + schedule[:-1], schedule)]
    assert sum(1 for n in retired_in if n > 0) >= 2, ("tiles retire in at least two different rounds", retired_in)
    # the raw criterion at the same eps retires another set
    raw = ar.reference_run(o, case)[2][-1][2]
    assert not np.array_equal(raw, last["active"]), "the filtered criterion must differ from the raw one at this eps"
    print("raw criterion at the same eps: %d of %d tiles still active" % (raw.sum(), raw.size))
    # the filtered estimate is what decides: no tile retired by the all-equal rule carries the case
    assert sum(int(r["equal"].sum()) for r in rounds) < (total - schedule[-1])
    # no per-tile maximum of the filtered plane lies within relative 1e-6 of eps: the device runs the filter bit for bit, but so the test says why
    nearest = min(float(np.abs(w[np.isfinite(w)] / eps - 1.0).min()) for w in (ar.tile_max(r["flt_stderr"]) for r in rounds))
    print("nearest per-tile maximum of the filtered stderr to eps: %.3g relative" % nearest)
    assert nearest > 1e-6


def test_f32_takes_the_f64_schedule(request):
    a = adr.reference_run(_oracle(request, "f64"), adr.CASES[0])[3]
    b = adr.reference_run(_oracle(request, "f32"), adr.CASES[1])[3]
    assert [r["active"].tolist() for r in a] == [r["active"].tolist() for r in b]
    assert not np.array_equal(a[-1]["linear"], b[-1]["linear"])


@pytest.mark.parametrize("size,region", [((61, 37), None), ((203, 99), adr.REGION)], ids=["61x37", "203x99-region"])
def test_retirement_rule_on_hand_made_maps(size, region):
    nx, ny = size
    eps = 0.25
    local = adr.local_tiles(nx, ny, region)
    maps = adr.synthetic_maps(nx, ny, eps, region)
    assert len(maps) >= 6
    for what, m, want in maps:
        got = adr.retire(local.copy(), m, eps, region)
        assert np.array_equal(got, want), (what, np.argwhere(got != want).tolist())
        assert not (got & ~local).any()
        assert np.array_equal(adr.retire(got, m, eps, region), got), (what, "a second identical call retires nothing")
    by = {w: (m, a) for w, m, a in maps}
    assert not by["exactly eps passes"][1].any() and by["everything fails"][1].sum() == local.sum()
    m, a = by["nextafter(eps, inf) fails"]
    assert (m > eps).sum() == 4 and a.sum() == 4  # the four corners of the region: partial tiles at the right and bottom edge
    m, a = by["NaN and +inf fail, -inf and negative values pass"]
    assert np.isnan(m).sum() == 2 and a.sum() == 3 and np.isneginf(m).sum() == 1
    m, a = by["one bad pixel per tile, every position"]
    assert 0 < a.sum() < local.sum()
    if region is not None:
        m, a = by["bad pixels outside the region are ignored"]
        assert np.isnan(m).sum() > 0 and not a.any()
        x0, y0, x1, y1 = region
        assert x0 % 8 and y0 % 8 and x1 % 8 and y1 % 8, "the region cuts tiles on every side"
    else:
        assert nx % 8 and ny % 8, "partial tiles at the right and bottom edge"
    # retirement is permanent: a tile that is not active is not looked at again
    none = np.zeros_like(local)
    assert not adr.retire(none, np.full((ny, nx), np.inf), eps, region).any()


# ---- the C-ABI, the binding and the Clojure host -------------------------------------------------------------------------------------------------
def test_retire_prototypes_parse_and_are_bound():
    protos = header_prototypes()
    assert protos["rtmi_adaptive_retire"] == ["handle", "i32", "i32", "double[]", "f64", "int[]"]
    assert protos["rtmi_adaptive_retire_device"] == ["handle", "i32", "i32", "device-pointer", "f64", "int[]", "device-pointer"]
    assert set(NAMES) <= set(_ffi.SYMBOLS)
    for name in ("adaptive_retire", "adaptive_retire_device"):
        assert callable(getattr(core.Context, name))
    assert callable(core.DeviceScene.refine_adaptive_denoised)


def test_library_exports_the_retire_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 208


def test_retire_checks_its_arguments_before_the_handle():
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    m = np.zeros((8, 8))
    p = m.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int32(7)
    for args, word in (((8, 8, None, 0.1), "noise"), ((8, 8, p, -1.0), "eps"), ((8, 8, p, float("nan")), "eps"), ((8, 8, p, float("inf")), "eps"),
                       ((0, 8, p, 0.1), "nx"), ((8, -1, p, 0.1), "nx")):
        assert L.rtmi_adaptive_retire(None, *args, ctypes.byref(n)) == RTMI_E_ARG and word in err(), args
        assert L.rtmi_adaptive_retire_device(None, *args, ctypes.byref(n), None) == RTMI_E_ARG and word in err(), args
    assert L.rtmi_adaptive_retire(None, 8, 8, p, 0.1, ctypes.byref(n)) == RTMI_E_STATE and "context" in err()
    assert L.rtmi_adaptive_retire_device(None, 8, 8, p, 0.1, None, None) == RTMI_E_STATE and "context" in err()
    assert n.value == 7


def test_gpu_clj_calls_adaptive_retire():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert {"adaptive-retire", "render-adaptive-denoised"} <= set(by_name)
    called = {x[2].strip('"') for x in walk(by_name["render-adaptive-denoised"]) if is_list(x, "call-int")}
    assert {"rtmi_render_features", "rtmi_render_adaptive", "rtmi_denoise", "rtmi_adaptive_retire", "rtmi_adaptive_status"} <= called
    assert "create-scene!" in {x[1] for x in walk(by_name["render-adaptive-denoised"]) if is_list(x)}
    assert {x[2].strip('"') for x in walk(by_name["adaptive-retire"]) if is_list(x, "call-int")} == {"rtmi_adaptive_retire"}
    # the device form takes device pointers, which the conformance reader cannot classify: it is bound on the Function itself
    assert "adaptive-retire-device" in by_name and '"rtmi_adaptive_retire_device"' in {x for x in walk(by_name["adaptive-retire-device"]) if isinstance(x, str)}


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--adaptive-denoised", "-1"], ["--adaptive-denoised", "nan"], ["--adaptive-denoised", "abc"],
                                   ["--adaptive-denoised"], ["--adaptive-denoised", "inf"], ["--adaptive-denoised=-0.5"],
                                   ["--adaptive-denoised", "0.1", "--noise", "0.1"], ["--noise=0.1", "--adaptive-denoised=0.1"],
                                   ["--adaptive-denoised", "0.1", "--adaptive", "0.1"], ["--adaptive=0.1", "--adaptive-denoised", "0.1"],
                                   ["--adaptive-denoised", "0.1", "--chunk", "0"], ["--adaptive-denoised", "0.1", "--denoise", "9"],
                                   ["--adaptive-denoised", "0.1", "--feature-samples", "0"]])
def test_cli_rejects_bad_adaptive_denoised_flags_before_device_work(tmp_path, monkeypatch, flags):
    touched = []
    monkeypatch.setattr(core, "DeviceScene", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(core, "render", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(_ffi, "lib", lambda: touched.append(1))
    out = tmp_path / "x.ppm"
    with pytest.raises(SystemExit):
        core.main([str(out), "8", "8", "4"] + flags)
    assert not touched and not out.exists()


def test_cli_flag_parser():
    assert core._adaptive_denoised_flags(["a.png", "8", "8"]) == (["a.png", "8", "8"], None)
    assert core._adaptive_denoised_flags(["a.png", "--adaptive-denoised", "0.02", "8"]) == (["a.png", "8"], 0.02)
    assert core._adaptive_denoised_flags(["--adaptive-denoised=0", "--chunk", "4", "--budget=2"]) == (["--chunk", "4", "--budget=2"], 0.0)


def test_cli_implies_denoise_with_the_defaults(tmp_path, monkeypatch):
    """the flags reach the driver: --denoise implied with the default passes, --feature-samples alone accepted, both as given otherwise"""
    seen = []

    class Stop(Exception):
        pass

    class FakeScene:
        def __init__(self, *a, **k):
            self.ctx = self

        def refine_adaptive_denoised(self, nx, ny, ns, chunk, eps, **kw):
            seen.append((nx, ny, ns, chunk, eps, kw))
            raise Stop

        def progressive_release(self):
            pass

        def close(self):
            pass

    monkeypatch.setattr(core, "DeviceScene", FakeScene)
    for flags, want in ((["--adaptive-denoised", "0.02"], (16, 0.02, dict(na=4, iterations=5))),
                        (["--adaptive-denoised=0.5", "--feature-samples", "2"], (16, 0.5, dict(na=2, iterations=5))),
                        (["--adaptive-denoised", "0.5", "--denoise", "3", "--chunk", "8"], (8, 0.5, dict(na=4, iterations=3))),
                        (["--denoise=2", "--feature-samples=1", "--adaptive-denoised", "1"], (16, 1.0, dict(na=1, iterations=2)))):
        with pytest.raises(Stop):
            core.main([str(tmp_path / "x.ppm"), "8", "8", "40", "two-spheres"] + flags)
        assert seen[-1] == (8, 8, 40) + want[:2] + (want[2],), flags
