"""The library's host half under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, on the CPU.

`make -C raytrace_clj_amd/csrc sanitize` compiles rtmi.hip twice with the host side instrumented (the floating-point flags are the shipped build's, so the
tables hash as librtmi.so's) and links each object with tests/host_san/driver.cpp, a stand-alone program that calls only the hooks include/rtmi.h documents as
host code only.  Every test writes a case file (tests/san_cases.py, from the inputs the host tests already build), runs a driver as a child process that
sees no device, and asks three things of the run: it exits 0, the sanitizers report nothing, and every line it prints is the line computed here from the
ordinary librtmi.so with the same arrays -- the sanitized build computes the same bits, it does not merely survive.  The oracle (oracle/rt_oracle.c) gets
the same treatment through oracle/san_main.c.  Nothing sanitized is loaded into this process, and nothing here needs or opens a GPU."""
import os
import shutil
import subprocess
import time

import pytest

from raytrace_clj_amd import _ffi
import san_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytrace_clj_amd", "csrc")
SAN_DIR = os.path.join(ROOT, "build", "san")
SANITIZERS = ("asan", "tsan")  # asan: -fsanitize=address,undefined
OPTIONS = {
    "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:strict_string_checks=1",
    "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
    "TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1",
}
REPORTS = ("ERROR: AddressSanitizer", "runtime error:", "WARNING: ThreadSanitizer", "LeakSanitizer")
# seconds a driver run may take: three times the slowest run measured for the group, rounded up to a whole second (TSan's slowdown varies with load).
# Measured, asan / tsan: trees 0.09 / 1.10, geometry 0.09 / 1.13, materials 0.04 / 0.03, refit 0.52 / 1.48, lights 0.04 / 0.03, scalars 0.04 / 0.03,
# errors 0.05 / 0.03, four callers at once 2.46 / 4.02, the size sweep 0.06 / 0.05, geometry and refit under a knob 0.61 / 1.75, a control 0.04 / 0.08, the oracle 0.10 / 0.41
TIMEOUT = {"trees": 4, "geometry": 4, "materials": 1, "refit": 5, "lights": 1, "scalars": 1, "errors": 1, "together": 13, "control": 1, "oracle": 2, "knobs": 6, "sizes": 1}
HOOKS = {"build_tree": "rtmi_test_build_tree", "pack_materials": "rtmi_test_pack_materials", "pack_geometry": "rtmi_test_pack_geometry",
         "refit": "rtmi_test_refit", "scene_lights": "rtmi_test_scene_lights", "stage_layout": "rtmi_test_stage_layout",
         "halves": "rtmi_test_half_outward rtmi_test_refit_half", "camera_fixed": "rtmi_test_camera_fixed", "sample_keys": "rtmi_sample_key",
         "version": "rtmi_version"}
HOST_ONLY = ("rtmi_test_build_tree", "rtmi_test_pack_materials", "rtmi_test_pack_geometry", "rtmi_test_refit", "rtmi_test_scene_lights", "rtmi_test_stage_layout",
             "rtmi_test_half_outward", "rtmi_test_refit_half", "rtmi_test_camera_fixed", "rtmi_version", "rtmi_last_error", "rtmi_sample_key")


@pytest.fixture(scope="module")
def drivers():
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is missing: the sanitized builds of the host half need it")
    t0 = time.time()
    done = subprocess.run(["make", "-j2", "-C", CSRC, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print("make sanitize: %.1f s" % (time.time() - t0))
    assert done.returncode == 0, "the sanitized builds failed:\n" + done.stdout[-4000:]
    return {san: os.path.join(SAN_DIR, "driver_" + san) for san in SANITIZERS}


def run_driver(path, args, timeout):
    """one driver run as a child process that finds no device -> (exit code, stdout lines, stderr, seconds)"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", **OPTIONS)
    t0 = time.time()
    done = subprocess.run([path] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace", env=env, timeout=timeout)
    return done.returncode, done.stdout.splitlines(), done.stderr, time.time() - t0


def assert_clean(code, err):
    assert not any(mark in err for mark in REPORTS), "a sanitizer reported:\n" + err[-6000:]
    assert code == 0, "the driver exited %d:\n%s" % (code, err[-2000:])


@pytest.fixture(scope="module")
def lib():
    return _ffi.lib()


@pytest.fixture(scope="module")
def scenes():
    return sc._scenes()


@pytest.fixture(scope="module")
def groups(lib, scenes):
    """group -> (calls, the lines the ordinary library gives), each built once for both sanitizers"""
    made = {}

    def count_lights(f):
        line = sc.expected_line(lib, sc.lights_call("count", f, 0))
        return int(line.split(" count=")[1].split(" ")[0])

    makers = {"trees": sc.tree_cases, "geometry": lambda: sc.geometry_cases(scenes), "materials": lambda: sc.material_cases(scenes), "refit": sc.refit_cases,
              "lights": lambda: sc.light_cases(count_lights), "sizes": sc.size_sweep_cases, "scalars": sc.scalar_cases, "errors": lambda: sc.error_cases(scenes)}

    def get(name):
        if name not in made:
            calls = makers[name]()
            made[name] = (calls, [sc.expected_line(lib, c) for c in calls])
        return made[name]
    return get


GROUPS = ("errors", "geometry", "lights", "materials", "refit", "scalars", "sizes", "trees")


def check_group(drivers, groups, tmp_path, name, san):
    calls, want = groups(name)
    assert len(calls) == len(want) > 0 and len({c.label for c in calls}) == len(calls), "labels are unique"
    path = str(tmp_path / (name + ".cases"))
    sc.write_cases(path, calls)
    code, have, err, seconds = run_driver(drivers[san], [path], TIMEOUT[name])
    print("%s under %s: %d driver lines compared, %.2f s" % (name, san, len(want), seconds))
    assert_clean(code, err)
    assert len(have) == len(want)
    for h, w in zip(have, want):
        assert h == w
    return calls, want


@pytest.mark.parametrize("san", SANITIZERS)
@pytest.mark.parametrize("name", [g for g in GROUPS if g != "errors"])
def test_hooks_compute_the_ordinary_librarys_bits_and_report_nothing(drivers, groups, tmp_path, name, san):
    calls, want = check_group(drivers, groups, tmp_path, name, san)
    for c, line in zip(calls, want):
        assert " rc=" not in line or " rc=0" in line, "a case of this group is refused: " + line


@pytest.mark.parametrize("san", SANITIZERS)
def test_error_paths_give_the_same_code_and_text_and_write_nothing(drivers, groups, tmp_path, san):
    """every refused input gives the code rtmi.h documents for it -- per packer and per way --, the ordinary library's text, and leaves the pattern in
    every output: scalars, lists and the whole buffers of the refit"""
    calls, want = check_group(drivers, groups, tmp_path, "errors", san)
    refused = 0
    for c, line in zip(calls, want):
        label, kind, fields, text = sc.line_fields(line)
        assert (label, kind) == (c.label, c.kind)
        assert int(fields["rc"]) == (0 if c.fails is False else c.fails), line
        if c.fails is False:  # (the edit's way of the material packer, which does not read what is wrong here)
            assert text is None and not sc.wrote_nothing(line, c), line
            continue
        refused += 1
        assert text, "a refused call says why: " + line
        assert sc.wrote_nothing(line, c), "a refused call wrote: " + line
    assert refused >= 120


def test_wrote_nothing_tells_a_written_output_from_the_pattern():
    """the check above can fail: lines whose outputs are not the pattern are rejected, field by field, whatever the error text holds"""
    fill32, fill64 = "-1515870811", "a5a5a5a5a5a5a5a5"
    tree = sc.Call("build_tree", "x", sc.E_ARG)
    assert sc.wrote_nothing("x build_tree rc=-1 hash=%s info=[%s,%s,%s,%s] err=bad arguments" % ((fill64,) + (fill32,) * 4), tree)
    assert sc.wrote_nothing("x build_tree rc=-1 hash=%s info=[%s,%s,%s,%s] err=text with hash=0 in it" % ((fill64,) + (fill32,) * 4), tree)
    assert not sc.wrote_nothing("x build_tree rc=-1 hash=0000000000000000 info=[%s,%s,%s,%s] err=bad" % ((fill32,) * 4), tree)
    assert not sc.wrote_nothing("x build_tree rc=-1 hash=%s info=[%s,%s,3,%s] err=bad" % (fill64, fill32, fill32, fill32), tree)
    assert not sc.wrote_nothing("x build_tree rc=-1 err=no output reported", tree)
    refit = sc.Call("refit", "y", sc.E_ARG, capacity=7, cells_capacity=2, leaf_floats=6, want_big=1)
    pat = lambda n: "%016x" % sc.fnv1a(bytes([sc.PATTERN]) * n)  # noqa: E731
    good = dict(bytes="-6510615555426900571", info="[%s]" % ",".join([fill32] * 10), big="[%s]" % ",".join([fill32] * 16), nodes=pat(7), cells=pat(8), leaf_box=pat(24))
    line = lambda f: "y refit rc=-1 " + " ".join("%s=%s" % kv for kv in f.items()) + " err=bad arguments"  # noqa: E731
    assert sc.wrote_nothing(line(good), refit)
    for key, other in (("bytes", "5"), ("info", "[0,0]"), ("big", "[1]"), ("nodes", pat(6)), ("cells", pat(7)), ("leaf_box", "%016x" % sc.fnv1a(b"\0" * 24))):
        assert not sc.wrote_nothing(line(dict(good, **{key: other})), refit), key
    layout = sc.Call("stage_layout", "z", sc.E_ARG, n=1)
    assert sc.wrote_nothing("z stage_layout rc=-1 total=%s offsets=null err=bad arguments" % fill64, layout)
    assert not sc.wrote_nothing("z stage_layout rc=-1 total=%s offsets=[%s,10] err=bad arguments" % (fill64, fill64), layout)
    assert sc.line_fields("a b rc=-3 hash=1 err=kind 9 unsupported: x=1")[3] == "kind 9 unsupported: x=1"


KNOBS = ({"RTMI_NODE16": "0"}, {"RTMI_NODE16": "1"}, {"RTMI_BOX_LEAF": "1"}, {"RTMI_MLOC": "1"}, {"RTMI_GRID": "0"})
_knob_cases = {}


@pytest.mark.parametrize("san", SANITIZERS)
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()))
def test_build_knobs_take_the_packers_and_the_refit_down_their_other_paths(drivers, lib, scenes, tmp_path, monkeypatch, knobs, san):
    """the builder's experiment knobs are read from the environment at every call: both node record sizes, Box leaves (one leaf record over six faces), the
    media's neighbourhood trees and a build without the entry grid -- other record arrays, other sizes -- over the geometry and the refit cases"""
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    key = tuple(sorted(knobs.items()))
    if key not in _knob_cases:  # (the sizing calls and the expected lines are made under the knobs too)
        calls = sc.geometry_cases(scenes) + sc.refit_cases()
        _knob_cases[key] = (calls, [sc.expected_line(lib, c) for c in calls])
    calls, want = _knob_cases[key]
    path = str(tmp_path / "knobs.cases")
    sc.write_cases(path, calls)
    code, have, err, seconds = run_driver(drivers[san], [path], TIMEOUT["knobs"])
    print("geometry + refit with %r under %s: %d driver lines compared, %.2f s" % (knobs, san, len(want), seconds))
    assert_clean(code, err)
    assert have == want
    assert all(" rc=0" in line for line in want)


def test_the_one_short_buffers_report_the_size_and_stay_untouched(groups):
    """rtmi_test_refit with one byte less than the node array needs: *out_bytes is the need, the node buffer keeps the pattern; the grid's cells are cut
    at the capacity (the driver allocates exactly that much: a longer copy is an ASan report)"""
    calls, want = groups("refit")
    by_label = {c.label: (c, line) for c, line in zip(calls, want)}
    n = 0
    for label, (c, line) in by_label.items():
        if not label.endswith("/one-short"):
            continue
        full = by_label[label.replace("/one-short", "/all-outputs")][1]
        need = int(full.split(" bytes=")[1].split(" ")[0])
        assert c.num("capacity") == need - 1 and int(line.split(" bytes=")[1].split(" ")[0]) == need
        # (a scene whose trees hold no node record needs 0 bytes: one short of that is no buffer at all)
        assert line.split(" nodes=")[1].split(" ")[0] == ("%016x" % sc.fnv1a(bytes([sc.PATTERN]) * (need - 1)) if need > 1 else "null"), label
        assert line.split(" info=")[1].split(" ")[0] == full.split(" info=")[1].split(" ")[0]
        n += 1
    assert n >= 10


@pytest.mark.parametrize("san", SANITIZERS)
@pytest.mark.parametrize("name", ["trees", "mixed"])
def test_four_callers_at_once_get_the_single_threaded_results(drivers, lib, scenes, tmp_path, name, san):
    """four threads start together behind a barrier and make three calls each -- team builds, a build on the calling thread alone, the geometry packer,
    a refit -- while the team is busy with someone else's: every result is the one the ordinary library gives a lone caller"""
    calls = sc.concurrent_cases(scenes)[name]
    want = [sc.expected_line(lib, c) for c in calls]
    path = str(tmp_path / "together.cases")
    sc.write_cases(path, calls)
    code, have, err, seconds = run_driver(drivers[san], [path, "--threads", 4, 3], TIMEOUT["together"])
    print("together/%s under %s: %d driver lines compared, %.2f s" % (name, san, len(have), seconds))
    assert_clean(code, err)
    assert have == ["t%d.r%d %s" % (t, k, want[t]) for t in range(4) for k in range(3)]


@pytest.mark.parametrize("san,what,report", [("asan", "heap", "ERROR: AddressSanitizer: heap-buffer-overflow"), ("asan", "ub", "runtime error: signed integer overflow"),
                                             ("tsan", "race", "WARNING: ThreadSanitizer: data race")])
def test_controls_a_deliberate_defect_in_the_driver_is_reported_and_fatal(drivers, san, what, report):
    """what shows that the instrumentation, the options, -fno-sanitize-recover and the link order are in effect: the driver's own defect, no library code"""
    code, out, err, _ = run_driver(drivers[san], ["--control", what], TIMEOUT["control"])
    assert code != 0 and report in err, (code, err[-2000:])
    assert "driver.cpp" in err  # the report names the line


def test_the_librarys_own_object_is_instrumented(drivers):
    """the controls show the driver's instrumentation; the library's object must carry the runtimes' entry points too (-Xarch_host reached the host half)"""
    for san, names in (("asan", (b"__asan_report_load", b"__ubsan_handle_")), ("tsan", (b"__tsan_read", b"__tsan_write", b"__tsan_func_entry"))):
        obj = open(os.path.join(SAN_DIR, "rtmi_%s.o" % san), "rb").read()
        for name in names:
            assert name in obj, (san, name)


def test_every_host_only_entry_has_a_case(groups, scenes):
    kinds, lines = set(), 0
    for name in GROUPS:
        calls, want = groups(name)
        kinds |= {c.kind for c in calls}
        lines += len(want)
    together = sc.concurrent_cases(scenes)
    lines += sum(3 * len(v) for v in together.values())
    under_knobs = len(KNOBS) * (len(groups("geometry")[0]) + len(groups("refit")[0]))
    print("driver lines compared per sanitizer: %d, and %d more under the build knobs" % (lines, under_knobs))
    covered = set(" ".join(HOOKS[k] for k in kinds).split()) | {"rtmi_last_error"}  # (every refused call prints its text)
    assert covered == set(HOST_ONLY)
    src = open(os.path.join(ROOT, "tests", "host_san", "driver.cpp")).read()
    called = {w.split("(")[0] for w in src.replace("\n", " ").split() if w.startswith("rtmi_") and "(" in w}
    assert called <= set(HOST_ONLY), "the driver calls only entries documented as host code only: %r" % sorted(called - set(HOST_ONLY))
    assert "hip/hip_runtime" not in src and "dlopen" not in src


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_drivers():
    if not shutil.which(os.environ.get("CC") or "cc"):
        pytest.skip("no C compiler: the sanitized builds of the oracle need one")
    done = subprocess.run(["make", "-j2", "-C", os.path.join(ROOT, "oracle"), "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, "the sanitized builds of the oracle failed:\n" + done.stdout[-4000:]
    return {san: os.path.join(ROOT, "oracle", "san_" + san) for san in SANITIZERS}


@pytest.fixture(scope="module")
def oracle_lines(oracle):
    calls = sc.oracle_cases(oracle)
    return calls, [sc.oracle_expected_line(oracle, c) for c in calls]


@pytest.mark.parametrize("san", SANITIZERS)
def test_oracle_computes_the_ordinary_librarys_bits_and_reports_nothing(oracle_drivers, oracle_lines, tmp_path, san):
    """frames of the golden scenes on 1 and 16 threads (32-pixel chunks dealt by an atomic counter), and hits, paths, cameras, textures and scatters"""
    calls, want = oracle_lines
    assert len({c.label for c in calls}) == len(calls) and {c.kind for c in calls} == {"render", "probe_hit", "probe_paths", "probe_camera", "probe_texture", "probe_scatter"}
    path = str(tmp_path / "oracle.cases")
    sc.write_cases(path, calls)
    code, have, err, seconds = run_driver(oracle_drivers[san], [path], TIMEOUT["oracle"])
    print("oracle under %s: %d driver lines compared, %.2f s" % (san, len(want), seconds))
    assert_clean(code, err)
    assert len(have) == len(want)
    for h, w in zip(have, want):
        assert h == w
    frames = {}
    for line in want:
        if " render " in line:  # 1 and 16 threads agree
            frames.setdefault(line.split("/threads=")[0], set()).add(line.split(" render ")[1])
    assert len(frames) == 3 and all(len(v) == 1 for v in frames.values()), frames
