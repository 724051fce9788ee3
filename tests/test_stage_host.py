"""CPU tests of the host forms' staging arena (HostIo in rtmi.hip): rtmi_test_stage_layout lays planes out with the code every host form uses, so the
carving that was offset arithmetic inside each entry is checked here, without a device, for the plane lists of all of them at odd sizes: every
present plane starts on a multiple of 16 bytes, no two overlap, an absent plane takes no space, the total is no more than the padded sizes add up
to, and byte sizes past 2^32 neither wrap nor fail."""
import itertools

import numpy as np
import pytest

from raytrace_clj_amd import _ffi

ABSENT = np.iinfo(np.uint64).max
F64, U64, I32, U8 = 8, 8, 4, 1


def layout(planes):
    """planes: (element bytes, count, present) triples -> ([offset or None], total)"""
    elem, count, present = (np.array([p[k] for p in planes], dt) for k, dt in ((0, np.uint64), (1, np.uint64), (2, np.int32)))
    off, total = np.zeros(len(planes), np.uint64), np.zeros(1, np.uint64)
    p = _ffi.ptr
    _ffi.check(_ffi.lib().rtmi_test_stage_layout(len(planes), p(elem), p(count), p(present), p(off), p(total)))
    return [None if o == ABSENT else int(o) for o in off], int(total[0])


def frame(npx, want_err, want_cnt, want_smp):  # the frame host forms: linear, stderr, counters, samples, rgb8
    return [(F64, 3 * npx, 1), (F64, npx, want_err), (U64, 2, want_cnt), (I32, npx, want_smp), (U8, 3 * npx, 1)]


def denoise(n, se, feat, olin, oq, ose):
    return [(F64, 3 * n, 1), (F64, n, se), (F64, 8 * n, feat), (F64, 3 * n, olin), (U8, 3 * n, oq), (F64, n, ose)]


def reproject(n, pse, cse, olin, oq, ow, ose, cnt):
    return [(F64, 3 * n, 1), (F64, n, 1), (F64, n, pse), (F64, 8 * n, 1), (F64, 3 * n, 1), (F64, n, cse), (F64, 8 * n, 1),
            (F64, 3 * n, olin), (U8, 3 * n, oq), (F64, n, ow), (F64, n, ose), (U64, 2, cnt)]


def rays(n_groups, group, keys, state, out_rays):
    n = n_groups * group
    return [(F64, 7 * n, 1), (U64, n, keys), (F64, n_groups * _ffi.RAYS_REC, state), (F64, 3 * n_groups, 1), (F64, n_groups, 1), (U64, 2, 1),
            (F64, 3 * n, out_rays)]


def probe_paths(n, max_seg):  # rays, keys, rgb, segment counts, log lengths, the log
    return [(F64, 7 * n, 1), (U64, n, 1), (F64, 3 * n, 1), (U64, n, 1), (I32, n, 1), (F64, n * max_seg * _ffi.SEG_REC, max_seg > 0)]


NPX = 21 * 13
LAYOUTS = {}
for name, flags in (("render", (0, 1, 0)), ("progressive", (1, 0, 0)), ("adaptive", (1, 0, 1)), ("multi_adaptive", (1, 1, 1))):
    LAYOUTS["frame-" + name] = frame(NPX, *flags)
LAYOUTS["frame-region-5x3"] = frame(15, 1, 1, 1)
LAYOUTS["features"] = [(F64, 8 * NPX, 1), (U64, 2, 1)]
LAYOUTS["retire"] = [(F64, NPX, 1)]
for bits in itertools.product((0, 1), repeat=5):
    LAYOUTS["denoise-%d%d%d%d%d" % bits] = denoise(NPX, *bits)
for bits in ((1, 1, 1, 1, 1, 1, 1), (0, 0, 1, 1, 1, 0, 1), (0, 1, 0, 1, 0, 0, 0), (1, 0, 1, 0, 1, 0, 1), (0, 0, 0, 0, 0, 0, 0)):
    LAYOUTS["reproject-%d%d%d%d%d%d%d" % bits] = reproject(NPX, *bits)
for bits in itertools.product((0, 1), repeat=3):
    LAYOUTS["rays-5x3-keys%d-state%d-out%d" % bits] = rays(5, 3, *bits)
LAYOUTS["probe-hit-7"] = [(F64, 7 * 7, 1), (F64, 7 * 11, 1)]
LAYOUTS["probe-paths-7-log3"] = probe_paths(7, 3)
LAYOUTS["probe-paths-7-nolog"] = probe_paths(7, 0)
LAYOUTS["probe-rng-5"] = [(U64, 5, 1), (F64, 5, 1)]
# the largest frame check_reproject_args admits, 2^30 pixels x 30 doubles (+ rgb8 + counters): 240 GiB of planes, the double planes all past 2^32 bytes
LAYOUTS["reproject-2^30-pixels"] = reproject(1 << 30, 1, 1, 1, 1, 1, 1, 1)
LAYOUTS["rays-2^31-64"] = rays((1 << 31) - 64, 1, 1, 1, 1)


def pad16(b):
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_planes_are_aligned_disjoint_and_tight(name):
    planes = LAYOUTS[name]
    off, total = layout(planes)
    spans = []
    for (elem, count, present), o in zip(planes, off):
        if not present:
            assert o is None, "an absent plane has no place"
            continue
        assert o is not None and o % 16 == 0, (name, o)
        spans.append((o, o + elem * count))
    spans.sort()
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start, "planes overlap: one ends at %d, the next starts at %d" % (end, start)
    assert spans[-1][1] <= total
    assert total <= sum(pad16(elem * count) for elem, count, present in planes if present)  # no more than the padded sizes (so: exact arithmetic, no wrap)
    assert total >= sum(elem * count for elem, count, present in planes if present)


def test_absent_planes_take_no_space():
    """leaving an optional plane out gives the layout of the list without it"""
    for name, planes in LAYOUTS.items():
        present = [p for p in planes if p[2]]
        off, total = layout(planes)
        off_p, total_p = layout(present)
        assert [o for o in off if o is not None] == off_p and total == total_p, name


def test_sizes_past_2_to_32():
    off, total = layout(LAYOUTS["reproject-2^30-pixels"])
    n = 1 << 30
    assert total == 30 * 8 * n + 3 * n + 16  # twelve planes, all multiples of 16 bytes already
    assert off[-1] == total - 16 and off[1] == 3 * 8 * n
    assert all(b - a >= 3 * n for a, b in zip(off, off[1:]))  # (the smallest plane but the counters: rgb8)


def test_hook_arguments_and_empty_list():
    L = _ffi.lib()
    total = np.full(1, 7, np.uint64)
    assert L.rtmi_test_stage_layout(0, None, None, None, None, _ffi.ptr(total)) == 0 and total[0] == 0
    assert L.rtmi_test_stage_layout(1, None, None, None, None, _ffi.ptr(total)) == -1
    assert L.rtmi_test_stage_layout(-1, None, None, None, None, _ffi.ptr(total)) == -1
    assert "rtmi_test_stage_layout" in _ffi.SYMBOLS
