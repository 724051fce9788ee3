"""Occlusion rays generated on the device (rtmi_occlusion_hemisphere*, rtmi_occlusion_targets*, rtmi_ambient_occlusion*), the parts that need no GPU:
camera.hemisphere_rays_disk -- the numpy restatement of the hemisphere rule of include/rtmi.h --, the restatement helper tests/occlusion_reference.py,
and the C-ABI's prototypes and argument checks."""
import math
import os
import re

import numpy as np

from raytrace_clj_amd import _ffi, camera, util
from tests import occlusion_reference as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtmi_occlusion_hemisphere", "rtmi_occlusion_hemisphere_device", "rtmi_occlusion_targets", "rtmi_occlusion_targets_device",
           "rtmi_ambient_occlusion", "rtmi_ambient_occlusion_device")
E_ARG, E_STATE = -1, -5
HALF_Z = 0.8660254037844387  # sqrt(3/4) rounded up: (1/4 + 0) + z z rounds to a square root of exactly 1.0, so (1/2, 0, z) normalises to nn.x = 1/2 exactly


def _points_normals(n, seed=3):
    """unit and non-unit normals: the axes, |n.x| on both sides of 0.5 and exactly 0.5 after normalisation, negative components"""
    rng = np.random.default_rng(seed)
    normals = rng.normal(0, 1, (n, 3))
    normals[: n // 2] /= np.sqrt((normals[: n // 2] ** 2).sum(axis=1))[:, None]  # unit up to rounding
    normals[n // 2:] *= rng.uniform(0.1, 4.0, (n - n // 2, 1))                    # any length
    special = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
               [0.5, 0.0, HALF_Z], [-0.5, HALF_Z, 0.0],                              # nn.x = +-0.5 exactly: the second branch of the tangent
               [0.49999999999999994, 0.0, HALF_Z], [0.5000000000000001, 0.0, -HALF_Z],
               [2.0, -2.0, -2.0], [-0.3, -0.3, -0.3]]
    normals[:len(special)] = np.array(special, np.float64)
    return rng.normal(0, 5, (n, 3)), normals


def _unit(n):
    return n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------
def test_directions_are_unit_on_the_normals_side_and_lifted_from_the_disk():
    p, n = _points_normals(2000)
    nn = _unit(n)
    assert math.sqrt((0.25 + 0.0) + HALF_Z * HALF_Z) == 1.0 and math.sqrt((0.25 + HALF_Z * HALF_Z) + 0.0) == 1.0
    assert (nn[:, 0] == 0.5).any() and (nn[:, 0] == -0.5).any() and (np.abs(nn[:, 0]) < 0.5).any() and (np.abs(nn[:, 0]) > 0.5).any()
    rays = camera.hemisphere_rays_disk(p, n, 50, time=0.25)
    assert rays.shape == (2000 * 50, 7) and rays.dtype == np.float64
    assert np.array_equal(rays[:, 0:3], np.repeat(p, 50, axis=0)) and np.all(rays[:, 6] == 0.25)
    d = rays[:, 3:6]
    norm_err = np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max()
    cos = (np.repeat(nn, 50, axis=0) * d).sum(axis=1)
    # r^2 of every row's accepted disk point, found independently of hemisphere_rays_disk's loop: all candidates of the first rounds at once, the
    # first accepted one picked per row (and the scalar walk over draw_bits for the rows of the special normals)
    g, k = (a.ravel() for a in np.meshgrid(np.arange(2000), np.arange(50), indexing="ij"))
    keys = util.sample_keys(0x5EED0002, g, k)
    rounds = 64
    cx = np.stack([2.0 * util.draw_uniforms(keys, 2 * c) - 1.0 for c in range(rounds)])
    cy = np.stack([2.0 * util.draw_uniforms(keys, 2 * c + 1) - 1.0 for c in range(rounds)])
    r2 = cx * cx + cy * cy
    inside = ~(r2 >= 1.0)
    assert inside.any(axis=0).all(), "a stream rejected %d candidates in a row" % rounds
    r2 = r2[inside.argmax(axis=0), np.arange(len(keys))]
    for row in range(12 * 50):
        x, y, _ = _first_accepted(util.sample_key(0x5EED0002, row // 50, row % 50))
        assert r2[row] == x * x + y * y
    worst = float(np.abs(cos - np.sqrt(1.0 - r2)).max())
    print("| |d| - 1 | <= %.3g, | d.n - sqrt(1 - r^2) | <= %.3g over %d rows" % (norm_err, worst, len(cos)))
    assert norm_err < 1e-15 and worst < 1e-15 and (cos > 0.0).all()


def test_any_split_over_first_gives_the_rows_of_one_call():
    p, n = _points_normals(64)
    whole = camera.hemisphere_rays_disk(p, n, 12, seed=99).reshape(64, 12, 7)
    for cut in (1, 5, 11):
        a = camera.hemisphere_rays_disk(p, n, cut, first=0, seed=99).reshape(64, cut, 7)
        b = camera.hemisphere_rays_disk(p, n, 12 - cut, first=cut, seed=99).reshape(64, 12 - cut, 7)
        assert np.array_equal(np.concatenate([a, b], axis=1).view(np.uint64), whole.view(np.uint64))
    assert not np.array_equal(camera.hemisphere_rays_disk(p, n, 12, seed=100).reshape(64, 12, 7), whole)
    # the signature and the row order of hemisphere_rays, which stays what it was
    old = camera.hemisphere_rays(p, n, 12, seed=99)
    assert old.shape == (64 * 12, 7) and np.array_equal(old[:, 0:3], whole.reshape(-1, 7)[:, 0:3]) and not np.array_equal(old, whole.reshape(-1, 7))


def _first_accepted(key):
    """the reference's loop, one candidate at a time: (x, y, candidates rejected before it)"""
    c = 0
    while True:
        x = 2.0 * ((util.draw_bits(key, 2 * c) >> 11) * 2.0 ** -53) - 1.0
        y = 2.0 * ((util.draw_bits(key, 2 * c + 1) >> 11) * 2.0 ** -53) - 1.0
        if not ((x * x + y * y) + 0.0 * 0.0 >= 1.0):
            return x, y, c
        c += 1


def test_the_accepted_candidate_is_the_first_accepted():
    """about the normal (0, 0, 1) the frame is t = (0, -1, 0), b = (1, 0, 0): the direction is (y, -x, z), so the disk point can be read back"""
    n_keys, seed, first = 1000, 0xABCDEF, 5
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (n_keys, 1))
    rays = camera.hemisphere_rays_disk(np.zeros((n_keys, 3)), normals, 1, first=first, seed=seed)
    rejected = 0
    for g in range(n_keys):
        x, y, c = _first_accepted(util.sample_key(seed, g, first))
        rejected += c
        assert rays[g, 3] == y and rays[g, 4] == -x and rays[g, 5] == math.sqrt(1.0 - (x * x + y * y)), g
    assert 150 < rejected < 400  # (acceptance pi / 4: 1000 (4 / pi - 1) = 273 rejections are expected)


def test_directions_are_cosine_weighted():
    """E[cos] = 2 / 3 and Var[cos] = 1 / 2 - 4 / 9 = 1 / 18 under a cosine-weighted density: the mean of 10^5 directions within 5 standard errors"""
    n = np.array([[0.3, -1.2, 0.7]])
    rays = camera.hemisphere_rays_disk(np.zeros((1, 3)), n, 100000, seed=12345)
    cos = rays[:, 3:6] @ _unit(n)[0]
    se = math.sqrt((1.0 / 18.0) / 100000)
    print("mean cos = %.6f, 2/3 +- 5 se = %.6f +- %.6f" % (cos.mean(), 2.0 / 3.0, 5 * se))
    assert abs(float(cos.mean()) - 2.0 / 3.0) <= 5.0 * se


# ---- the restatement helper ----------------------------------------------------------------------------------------------------------------
def _records(n=40, seed=8):
    rng = np.random.default_rng(seed)
    hits = np.zeros((n, oref.HIT_REC))
    hits[:, 0] = 1.0
    hits[:, 3:6] = rng.normal(0, 3, (n, 3))
    hits[:, 6:9] = _unit(rng.normal(0, 1, (n, 3)))
    view = np.concatenate([rng.normal(0, 3, (n, 3)), rng.normal(0, 1, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1)
    return hits, view


def test_degenerate_records_yield_rows_of_zeros():
    hits, view = _records()
    hits[3, 6:9] = 0.0        # a zero normal
    hits[5, 4] = np.nan       # a non-finite point
    hits[6, 3] = -np.inf
    hits[9, 8] = np.inf       # a non-finite normal
    hits[11, 0] = 0.0         # a miss whose other columns hold something
    hits[12] = 0.0            # a miss as rtmi_query_hits writes it
    rays, ok = oref.hemisphere(hits, 4, view=view, first=2, seed=7)
    bad = [3, 5, 6, 9, 11, 12]
    assert np.array_equal(np.flatnonzero(~ok), bad)
    rows = rays.reshape(-1, 4, 7)
    assert not rows[bad].any() and np.isfinite(rays).all()
    good = np.flatnonzero(ok)
    assert np.array_equal(rows[good, :, 0:3], np.repeat(hits[good, None, 3:6], 4, axis=1)) and np.array_equal(rows[good, :, 6], np.repeat(view[good, 6:7], 4, axis=1))
    # the other points' rays do not move when a neighbour drops out: a point's index keys its streams
    clean, _ = _records()
    assert np.array_equal(oref.hemisphere(clean, 4, view=view, first=2, seed=7)[0].reshape(-1, 4, 7)[good], rows[good])
    # the targets rule reads no normal: points 3 and 9 send rays there
    tg = np.array([[0.0, 5.0, 0.0], [1.0, 2.0, 3.0]])
    trays, tok = oref.targets(hits, tg, time=0.5)
    assert np.array_equal(np.flatnonzero(~tok), [5, 6, 11, 12])
    t = trays.reshape(-1, 2, 7)
    assert not t[[5, 6, 11, 12]].any() and np.array_equal(t[3, 1, 3:6], tg[1] - hits[3, 3:6]) and (t[tok][:, :, 6] == 0.5).all()


def test_the_side_follows_the_view_ray():
    hits, view = _records()
    rays, ok = oref.hemisphere(hits, 8, view=view, seed=3)
    assert ok.all()
    d = rays[:, 3:6].reshape(-1, 8, 3)
    facing = (d * hits[:, None, 6:9]).sum(axis=2) > 0.0
    away = (hits[:, 6:9] * view[:, 3:6]).sum(axis=1) > 0.0
    assert away.any() and (~away).any()
    assert np.array_equal(facing, np.repeat(~away[:, None], 8, axis=1))          # the rays leave towards the viewer
    assert ((oref.hemisphere(hits, 8, seed=3)[0][:, 3:6].reshape(-1, 8, 3) * hits[:, None, 6:9]).sum(axis=2) > 0.0).all()  # without a view: the normal's side
    assert (oref.hemisphere(hits, 8, seed=3, time=0.75)[0][:, 6] == 0.75).all()


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------------------
def _lib():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    return _ffi.lib()


def _prototypes():
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(rtmi_(?:occlusion|ambient_occlusion)\w*)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_six_entries_and_the_library_exports_them():
    protos = _prototypes()
    assert sorted(protos) == sorted(ENTRIES)
    assert len(protos["rtmi_occlusion_hemisphere"]) == 15 and len(protos["rtmi_occlusion_targets"]) == 14 and len(protos["rtmi_ambient_occlusion"]) == 12
    L = _lib()
    for name in ENTRIES:
        assert protos[name][0].startswith("rtmi_scene") and name in _ffi.SYMBOLS
        assert len(getattr(L, name).argtypes) == len(protos[name]), name
        if name.endswith("_device"):
            assert protos[name][-1].replace(" ", "") == "void*stream" and len(protos[name]) == len(protos[name[:-7]]) + 1
    assert L.rtmi_version() >= 217
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "THE HEMISPHERE RULE" in header and "THE TARGETS RULE" in header


def test_argument_errors_come_before_the_handle():
    L = _lib()
    hits, cnt, tg = np.zeros((4, 12)), np.zeros(2, np.uint64), np.zeros((2, 3))
    p = _ffi.ptr
    big = 2 ** 31 - 63  # one more than the 2^31 - 64 rays a call may hold
    hemi = lambda n, h, nd, first: L.rtmi_occlusion_hemisphere(None, 0, n, h, None, nd, first, 1, 0.0, 0.001, 1.0, None, None, None, p(cnt))  # noqa: E731
    hemi_d = lambda n, h, nd, first: L.rtmi_occlusion_hemisphere_device(None, 0, n, h, None, nd, first, 1, 0.0, 0.001, 1.0, None, None, None, None, None)  # noqa: E731
    for f in (hemi, hemi_d):
        assert f(-1, p(hits), 4, 0) == E_ARG            # n_points < 0
        assert f(4, p(hits), 0, 0) == E_ARG             # n_dirs <= 0
        assert f(4, p(hits), 4, -1) == E_ARG            # first < 0
        assert f(4, None, 4, 0) == E_ARG                # NULL hits
        assert f(2 ** 30, p(hits), 4, 0) == E_ARG       # n_points * n_dirs overflows
        assert f(1, p(hits), big, 0) == E_ARG
        assert f(4, p(hits), 4, 0) == E_STATE           # sound arguments: the NULL handle is what is wrong
    targ = lambda n, h, nt, t: L.rtmi_occlusion_targets(None, 0, n, h, None, nt, t, 0.0, 0.001, 0.999, None, None, None, p(cnt))  # noqa: E731
    targ_d = lambda n, h, nt, t: L.rtmi_occlusion_targets_device(None, 0, n, h, None, nt, t, 0.0, 0.001, 0.999, None, None, None, None, None)  # noqa: E731
    for f in (targ, targ_d):
        assert f(-1, p(hits), 2, p(tg)) == E_ARG
        assert f(4, p(hits), 0, p(tg)) == E_ARG         # n_targets <= 0
        assert f(4, None, 2, p(tg)) == E_ARG            # NULL hits
        assert f(4, p(hits), 2, None) == E_ARG          # NULL targets
        assert f(2 ** 30, p(hits), 4, p(tg)) == E_ARG
        assert f(4, p(hits), 2, p(tg)) == E_STATE
    vis = np.zeros(16)
    ao = lambda nx, ny, nd, first, radius, v: L.rtmi_ambient_occlusion(None, 0, nx, ny, nd, first, radius, 1, v, None, None, p(cnt))  # noqa: E731
    ao_d = lambda nx, ny, nd, first, radius, v: L.rtmi_ambient_occlusion_device(None, 0, nx, ny, nd, first, radius, 1, v, None, None, None, None)  # noqa: E731
    for f in (ao, ao_d):
        assert f(-4, 4, 2, 0, 1.0, p(vis)) == E_ARG
        assert f(4, 4, 0, 0, 1.0, p(vis)) == E_ARG      # n_dirs <= 0
        assert f(4, 4, 2, -1, 1.0, p(vis)) == E_ARG     # first < 0
        assert f(4, 4, 2, 0, 0.0, p(vis)) == E_ARG      # radius <= 0
        assert f(4, 4, 2, 0, -1.0, p(vis)) == E_ARG
        assert f(4, 4, 2, 0, float("nan"), p(vis)) == E_ARG
        assert f(4, 4, 2, 0, 1.0, None) == E_ARG        # NULL out_visibility
        assert f(2 ** 15, 2 ** 15, 4, 0, 1.0, p(vis)) == E_ARG  # nx * ny * n_dirs overflows
        assert f(4, 4, 2, 0, 1.0, p(vis)) == E_STATE


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_ao_device_like_ao():
    import pytest

    from raytrace_clj_amd import core
    assert core._ao_flags(["out.png", "--ao-device", "8", "2.5", "40"], "--ao-device") == (["out.png", "40"], (8, 2.5))
    assert core._ao_flags(["--ao-device=4", "out.png"], "--ao-device") == (["out.png"], (4, 1.0))
    assert core._ao_flags(["--ao-device", "8", "out.png"]) == (["--ao-device", "8", "out.png"], None)  # --ao's own parse leaves it alone
    assert core._ao_flags(["--ao", "8", "out.png"]) == (["out.png"], (8, 1.0))                          # and --ao is what it was
    for bad in (["--ao-device"], ["--ao-device", "x"], ["--ao-device", "0"], ["--ao-device", "4", "0"]):
        with pytest.raises(SystemExit) as e:
            core._ao_flags(bad, "--ao-device")
        assert "--ao-device" in str(e.value)
    with pytest.raises(SystemExit) as e:
        core.main(["--ao", "4", "--ao-device", "4", "out.png"])
    assert "give one of them" in str(e.value)
