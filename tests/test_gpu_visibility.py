"""Closest-hit and any-hit queries on the device (rtmi_query_hits*, rtmi_query_occluded*).  The yardstick is rtmi_probe_hit, which the rest of the suite
pins to the CPU oracle: query_hits must write its record bit for bit, occluded must write its hit flag -- whatever the any-hit search met first -- for
every scene family, range, option and ray the recipes of tests/visibility_cases.py hold."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from raytrace_clj_amd import _ffi, camera, core
from raytrace_clj_amd import flatten as fl
from tests import tree_scenes as ts
from tests import visibility_cases as vc

FLT_MAX = vc.FLT_MAX
INCLUSIVE_KINDS = (fl.PRIM_RECT_XY, fl.PRIM_RECT_XZ, fl.PRIM_RECT_YZ, fl.PRIM_TRIANGLE)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


@functools.lru_cache(maxsize=None)
def _open(name):
    """one context and device scene per recipe for the whole module; a test that sets an option sets it back"""
    ctx = core.Context(0)
    return ctx, core.DeviceScene(vc.flat(name), ctx=ctx)


@functools.lru_cache(maxsize=None)
def _reference(name, t_min=0.001, t_max=FLT_MAX, precision="f64"):
    """probe_hit of the scene's ray set through the tree, computed once; do not write into it"""
    ctx, ds = _open(name)
    ctx.set_option("accel", 1)
    return ds.probe_hit(vc.rays(_oracle(), name), t_min, t_max, precision=precision)


def _check_records(ds, f, rays, exp, what, **kw):
    got, cnt = ds.query_hits(rays, return_counters=True, **kw)
    assert got.shape == (len(rays), _ffi.HIT_REC)
    assert _same(got[:, :11], exp), "%s: %d records differ from probe_hit's" % (what, (got[:, :11] != exp).any(axis=1).sum())
    hit = exp[:, 0] == 1
    mat = np.where(hit, np.asarray(f.prim_mat)[exp[:, 1].astype(np.int64)], 0)
    assert np.array_equal(got[:, 11], mat.astype(np.float64)), what + ": material"
    assert list(cnt) == [len(rays), int(hit.sum())], (what, list(cnt))
    return got


def _check_flags(ds, rays, exp_flags, what, group=1, **kw):
    flags, counts, cnt = ds.occluded(rays, group=group, **kw)
    assert flags.dtype == np.uint8 and _same(flags, exp_flags.astype(np.uint8)), "%s: %d flags differ" % (what, (flags != exp_flags).sum())
    assert np.array_equal(counts, exp_flags.reshape(-1, group).sum(axis=1).astype(np.int32)), what + ": group counts"
    assert list(cnt) == [len(rays), int(exp_flags.sum())], (what, list(cnt))


# ---- 1. records ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.SCENES)
def test_records_equal_probe_hit(name):
    ctx, ds = _open(name)
    f, rays = vc.flat(name), vc.rays(_oracle(), name)
    if name in ts.HOST_TABLE:
        assert ds.tree_info() == ts.HOST_TABLE[name], "the scene's tree is not the one this test is about"
    exp = _reference(name)
    assert (exp[:, 0] == 1).any()
    if name not in vc.MEDIA_SCENES:
        orc = _oracle().probe_hit(f, rays)
        assert np.array_equal(exp[:, :2], orc[:, :2]), "hit flag and primitive against the oracle"
    for accel in (0, 1):
        ctx.set_option("accel", accel)
        assert _same(ds.probe_hit(rays), exp)
        _check_records(ds, f, rays, exp, "%s accel %d" % (name, accel))
        if name in vc.SPHERE_SCENES:
            _check_records(ds, f, rays, ds.probe_hit(rays, precision="f32"), "%s accel %d f32" % (name, accel), precision="f32")
    ctx.set_option("accel", 1)


def test_f32_is_for_sphere_worlds_only():
    _, ds = _open("cornell")
    with pytest.raises(_ffi.RtmiError) as e:
        ds.query_hits(vc.rays(_oracle(), "cornell")[:8], precision="f32")
    assert e.value.code == -3
    with pytest.raises(_ffi.RtmiError) as e:
        ds.occluded(vc.rays(_oracle(), "cornell")[:8], precision="f32")
    assert e.value.code == -3


# ---- 2. flags -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.SCENES)
def test_flags_equal_the_closest_hit_searchs(name):
    ctx, ds = _open(name)
    rays = vc.rays(_oracle(), name)
    some = 0
    for t_min, t_max in vc.RANGES:
        exp = _reference(name, t_min, t_max)
        some += int(exp[:, 0].sum())
        for accel in (0, 1):
            ctx.set_option("accel", accel)
            what = "%s accel %d range (%g, %g)" % (name, accel, t_min, t_max)
            assert _same(ds.query_hits(rays, t_min, t_max)[:, :11], exp), what
            _check_flags(ds, rays, exp[:, 0], what, t_min=t_min, t_max=t_max)
    assert some > 0 and not _reference(name, *vc.RANGES[3])[:, 0].any()  # (an empty interval holds no hit)
    if name in vc.SPHERE_SCENES:
        for accel in (0, 1):
            ctx.set_option("accel", accel)
            _check_flags(ds, rays, ds.probe_hit(rays, precision="f32")[:, 0], name + " f32", precision="f32")
    ctx.set_option("accel", 1)


@pytest.mark.parametrize("name", ("cornell", "mixed(65)", "cloud(129)"))
def test_a_hit_at_exactly_t_max(name):
    """a rectangle or triangle hit at t == t-max is a hit (t <= t-max, hitable.clj:278, 564), a sphere hit there is none (t < t-max, :195): the ray's
    own closest t, from the probe, as its t-max -- nothing lies in front of it, so the flag is the primitive's own answer"""
    ctx, ds = _open(name)
    f, rays = vc.flat(name), vc.rays(_oracle(), name)
    exp = _reference(name)
    hit = exp[:, 0] == 1
    rays, t = rays[hit], exp[hit, 2]
    inclusive = np.isin(np.asarray(f.prim_kind)[exp[hit, 1].astype(np.int64)] & 15, INCLUSIVE_KINDS)
    assert inclusive.any() if name != "cloud(129)" else not inclusive.any()
    if name == "mixed(65)":
        assert (~inclusive).any()
    t_range = np.stack([np.full(len(t), 0.001), t], axis=1)
    for accel in (0, 1):
        ctx.set_option("accel", accel)
        flags = ds.occluded(rays, t_range=t_range)[0]
        assert np.array_equal(flags, inclusive.astype(np.uint8)), "%s accel %d" % (name, accel)
        assert np.array_equal(ds.query_hits(rays, t_range=t_range)[:, 0], inclusive.astype(np.float64))
        # one ulp further the sphere is in as well
        assert ds.occluded(rays, t_range=np.stack([t_range[:, 0], np.nextafter(t, np.inf)], axis=1))[0].all()
    ctx.set_option("accel", 1)


# ---- 3. per-ray ranges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover", "cornell", "layer(256)"))
def test_per_ray_ranges(name):
    ctx, ds = _open(name)
    rays = vc.rays(_oracle(), name)
    pairs = np.array(vc.RANGES[:3])
    which = np.arange(len(rays)) % 3
    t_range = pairs[which]
    got = ds.query_hits(rays, t_min=123.0, t_max=124.0, t_range=t_range)  # (the scalars are ignored)
    flags = ds.occluded(rays, t_min=123.0, t_max=124.0, t_range=t_range)[0]
    for k in range(3):
        exp = _reference(name, pairs[k, 0], pairs[k, 1])[which == k]
        assert _same(got[which == k, :11], exp), (name, k)
        assert np.array_equal(flags[which == k], exp[:, 0].astype(np.uint8)), (name, k)


# ---- 4. keys ------------------------------------------------------------------------------------------------------------------------------------
def test_keys_are_the_streams_the_media_draw_from():
    name = "hitlist-media"
    ctx, ds = _open(name)
    rays, keys = vc.rays(_oracle(), name), vc.keys()
    got = ds.query_hits(rays, keys=keys, ctr0=0)
    rgb, nseg, log, nlog = ds.probe_paths(rays, keys, depth=50, ctr0=0, max_seg=1)
    assert np.array_equal(got[:, 0], (nlog > 0).astype(np.float64))
    hit = nlog > 0
    assert hit.any() and _same(got[hit, 1:9], log[hit, 0, 0:8]), "prim, t, p, normal of the first logged segment"
    assert _same(ds.query_hits(rays)[:, :11], _reference(name))  # keys NULL: keyed 0, as probe_hit
    unkeyed = _reference(name)
    assert (got[:, 1] != unkeyed[:, 1]).any(), "the ray set never reaches a medium: the keys were not exercised"
    assert np.array_equal(ds.occluded(rays, keys=keys, ctr0=0)[0], got[:, 0].astype(np.uint8))
    later = ds.query_hits(rays, keys=keys, ctr0=3)
    assert np.array_equal(ds.occluded(rays, keys=keys, ctr0=3)[0], later[:, 0].astype(np.uint8))


# ---- 5. groups ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", (1, 7, 64, 100))
def test_group_counts(group):
    name = "cloud(129)"
    ctx, ds = _open(name)
    n_groups = vc.N // group
    rays = vc.rays(_oracle(), name)[:n_groups * group]
    exp = _reference(name, 0.001, 1.0)[:n_groups * group, 0]
    assert 0 < exp.sum() < len(exp)
    _check_flags(ds, rays, exp, "group %d" % group, group=group, t_max=1.0)


def test_empty_and_single_calls():
    name = "cloud(129)"
    ctx, ds = _open(name)
    rays = vc.rays(_oracle(), name)
    flags, counts, cnt = ds.occluded(rays[:0], group=5)
    assert len(flags) == 0 and len(counts) == 0 and list(cnt) == [0, 0]
    assert ds.query_hits(rays[:0]).shape == (0, _ffi.HIT_REC)
    exp = _reference(name)
    k = int(np.flatnonzero(exp[:, 0] == 1)[0])
    _check_flags(ds, rays[k:k + 1], exp[k:k + 1, 0], "one ray")
    _check_records(ds, vc.flat(name), rays[k:k + 1], exp[k:k + 1], "one ray")


# ---- 6. refill --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks_per_cu", (1, None))
def test_many_rays_refill_the_waves(blocks_per_cu):
    name, n = "cloud(129)", 200000
    ctx = core.Context(0)
    ds = core.DeviceScene(vc.flat(name), ctx=ctx)
    try:
        if blocks_per_cu is not None:
            ctx.set_option("blocks_per_cu", blocks_per_cu)
        reps = (n + vc.N - 1) // vc.N
        rays = np.tile(vc.rays(_oracle(), name), (reps, 1))[:n]
        exp = np.tile(_reference(name, 0.001, 4.0), (reps, 1))[:n]
        got, cnt = ds.query_hits(rays, t_max=4.0, return_counters=True)
        assert _same(got[:, :11], exp) and list(cnt) == [n, int(exp[:, 0].sum())]
        flags, counts, cnt = ds.occluded(rays, group=8, t_max=4.0)
        assert np.array_equal(flags, exp[:, 0].astype(np.uint8)) and list(cnt) == [n, int(exp[:, 0].sum())]
        assert np.array_equal(counts, exp[:, 0].reshape(-1, 8).sum(axis=1).astype(np.int32))
    finally:
        ds.close()
        ctx.close()


# ---- 7. options -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover", "cornell", "mixed(65)"))
def test_options_change_no_bit(name):
    ctx = core.Context(0)
    ds = core.DeviceScene(vc.flat(name), ctx=ctx)
    try:
        f, rays = vc.flat(name), vc.rays(_oracle(), name)
        exp = _reference(name)
        ctx.set_option("accel", 0)
        for variant in (0, 1, 2, 3):
            ctx.set_option("scan_variant", variant)
            _check_records(ds, f, rays, exp, "%s scan_variant %d" % (name, variant))
            _check_flags(ds, rays, exp[:, 0], "%s scan_variant %d" % (name, variant))
        ctx.set_option("accel", 1)
        for option, values in (("flat_below", (0, 24)), ("suspend_lanes", (0, 8))):
            for v in values:
                ctx.set_option(option, v)
                _check_records(ds, f, rays, exp, "%s %s %d" % (name, option, v))
                _check_flags(ds, rays, exp[:, 0], "%s %s %d" % (name, option, v))
    finally:
        ds.close()
        ctx.close()


# ---- 8. degenerate rays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover", "cornell", "layer(256)"))
def test_degenerate_rays(name):
    ctx, ds = _open(name)
    base = vc.rays(_oracle(), name)[:64].copy()
    rays = np.tile(base, (6, 1))
    rays[0:64, 3] = np.nan                      # a NaN direction component
    rays[64:128, 4] = np.inf                    # an infinite one
    rays[128:192, 3:6] = 0.0                    # no direction at all
    rays[192:256, 0] = -np.inf                  # an infinite origin
    rays[256:320, 0:3] += np.array([3e9, -2e9, 1e9])  # an origin far outside the scene's bound ...
    rays[320:384, 0:3] *= 1e17                  # ... and one the float traversal cannot hold
    rays = np.concatenate([rays, base])         # (and sound rays among them: the waves are mixed)
    order = np.random.default_rng(9).permutation(len(rays))
    rays = np.ascontiguousarray(rays[order])
    for accel in (0, 1):
        ctx.set_option("accel", accel)
        for t_min, t_max in ((0.001, FLT_MAX), (2.0, 1.0)):  # the second: t-min > t-max
            exp = ds.probe_hit(rays, t_min, t_max)
            what = "%s accel %d (%g, %g)" % (name, accel, t_min, t_max)
            assert _same(ds.query_hits(rays, t_min, t_max)[:, :11], exp), what
            assert np.array_equal(ds.occluded(rays, t_min=t_min, t_max=t_max)[0], exp[:, 0].astype(np.uint8)), what
    ctx.set_option("accel", 1)


# ---- 9. device forms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cover", "cornell"))
def test_device_forms_on_a_side_stream(name):
    import torch
    ctx, ds = _open(name)
    rays = vc.rays(_oracle(), name)
    n, group = 2996, 7
    exp = _reference(name, 0.001, 2.0)[:n]
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays[:n]).to(dev)
    d_range = torch.from_numpy(np.tile(np.array([0.001, 2.0]), (n, 1))).to(dev)
    d_hits = torch.full((n, _ffi.HIT_REC), -1.0, dtype=torch.float64, device=dev)
    d_flags = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_counts = torch.full((n // group,), 7, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(6, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    handle = int(side.cuda_stream)

    def calls():
        ds.query_hits_device(n, d_rays, d_hits, t_range=d_range, out_counters=d_cnt[0:2], stream=handle)
        ds.occluded_device(n // group, group, d_rays, out_occluded=d_flags, t_min=0.001, t_max=2.0, out_counters=d_cnt[2:4], stream=handle)
        ds.occluded_device(n // group, group, d_rays, out_count=d_counts, t_range=d_range, out_counters=d_cnt[4:6], stream=handle)
        side.synchronize()

    calls()
    bytes_before = np.zeros(1, np.int64)
    _ffi.check(_ffi.lib().rtmi_scene_device_bytes(ds.handle, bytes_before.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    free_before = torch.cuda.mem_get_info(dev)[0]
    d_hits.fill_(-1.0); d_flags.fill_(7); d_counts.fill_(7)
    torch.cuda.synchronize(dev)
    calls()
    bytes_after = np.zeros(1, np.int64)
    _ffi.check(_ffi.lib().rtmi_scene_device_bytes(ds.handle, bytes_after.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    assert bytes_after[0] == bytes_before[0] and torch.cuda.mem_get_info(dev)[0] == free_before, "the second call allocated"
    host = ds.query_hits(rays[:n], 0.001, 2.0)
    assert _same(d_hits.cpu().numpy(), host) and _same(host[:, :11], exp)
    flags = exp[:, 0].astype(np.uint8)
    assert np.array_equal(d_flags.cpu().numpy(), flags)
    assert np.array_equal(d_counts.cpu().numpy(), flags.reshape(-1, group).sum(axis=1).astype(np.int32))
    assert d_cnt.cpu().numpy().tolist() == [n, int(flags.sum())] * 3
    assert handle != 0


# ---- 10. the exit is real -----------------------------------------------------------------------------------------------------------------------
def test_any_hit_visits_less_of_the_tree():
    orc = _oracle()
    rays, f = vc.count_rays(orc), vc.count_flat()
    ctx = core.Context(0)
    ds = core.DeviceScene(f, ctx=ctx)
    try:
        assert ds.tree_info()[2] > 0, "the layer has no entry grid: not the scene this test is about"
        ctx.set_option("accel", 1)
        exp = ds.probe_hit(rays)
        assert np.array_equal(exp[:, :2], orc.probe_hit(f, rays)[:, :2]) and exp[:, 0].mean() >= 0.5
        ctx.set_option("count_traversal", 1)
        assert _same(ds.query_hits(rays)[:, :11], exp)
        closest = ctx.last_traversal_counters()
        flags = ds.occluded(rays)[0]
        any_hit = ctx.last_traversal_counters()
        print("AABB + primitive tests: closest hit %d + %d, any hit %d + %d" % (closest + any_hit))
        assert np.array_equal(flags, exp[:, 0].astype(np.uint8))
        assert 0 < sum(any_hit) < sum(closest)
    finally:
        ds.close()
        ctx.close()


# ---- 11. pick and ambient_occlusion ---------------------------------------------------------------------------------------------------------------
def test_pick_returns_what_probe_hit_sees():
    ctx, ds = _open("cornell")
    f = vc.flat("cornell")
    nx = ny = 48
    seen = set()
    for i, j in ((24, 24), (3, 40), (44, 5), (24, 46), (10, 20)):
        ray = ds.pixel_centre_rays(nx, ny, [i], [j])
        exp = ds.probe_hit(ray)[0]
        got = ds.pick(nx, ny, i, j)
        if exp[0] == 0:
            assert got is None
            continue
        assert got["prim"] == int(exp[1]) and got["material"] == int(np.asarray(f.prim_mat)[int(exp[1])]) and got["t"] == exp[2]
        assert np.array_equal(got["p"], exp[3:6]) and np.array_equal(got["normal"], exp[6:9]) and np.array_equal(got["uv"], exp[9:11])
        seen.add(got["prim"])
    assert len(seen) >= 2
    # the centre ray of a frame's pixel: where the pinhole of a zero-aperture lens looks
    centre = ds.pixel_centre_rays(nx, ny)
    assert centre.shape == (nx * ny, 7) and np.array_equal(centre[24 * nx + 24], ds.pixel_centre_rays(nx, ny, [24], [24])[0])


def _ao_by_probe(ds, nx, ny, n_dirs, radius, seed):
    primary = ds.pixel_centre_rays(nx, ny)
    h = ds.probe_hit(primary)
    hit = h[:, 0] == 1
    normals = h[:, 6:9].copy()
    away = (normals * primary[:, 3:6]).sum(axis=1) > 0.0
    normals[away] = -normals[away]
    normals[~hit] = (0.0, 1.0, 0.0)
    sec = camera.hemisphere_rays(h[:, 3:6], normals, n_dirs, seed=seed, time=primary[0, 6])
    occ = ds.probe_hit(sec, 0.001, radius)[:, 0].reshape(-1, n_dirs).sum(axis=1)
    vis = 1.0 - occ / float(n_dirs)
    vis[~hit] = 1.0
    return vis.reshape(ny, nx), hit.reshape(ny, nx)


def test_ambient_occlusion_is_the_fold_of_probe_flags():
    ctx, ds = _open("cover")
    nx, ny, n_dirs = 32, 16, 8
    exp, _ = _ao_by_probe(ds, nx, ny, n_dirs, 1.0, core.RENDER_SEED)
    got = ds.ambient_occlusion(nx, ny, n_dirs, 1.0)
    assert got.shape == (ny, nx) and np.array_equal(got, exp)
    assert 0.0 < got.mean() < 1.0 and got.min() < 1.0
    assert np.array_equal(ds.ambient_occlusion(nx, ny, n_dirs, 1.0, chunk=3), exp)  # any split of the directions


def test_ambient_occlusion_is_one_on_sky_pixels():
    ctx = core.Context(0)
    ds = core.DeviceScene(vc.count_flat(), ctx=ctx)  # the layer without a dome: the pixels above the horizon see nothing
    try:
        nx, ny, n_dirs = 32, 16, 4
        exp, hit = _ao_by_probe(ds, nx, ny, n_dirs, 0.5, 77)
        got = ds.ambient_occlusion(nx, ny, n_dirs, 0.5, seed=77)
        assert (~hit).any() and hit.any()
        assert np.array_equal(got, exp) and (got[~hit] == 1.0).all()
    finally:
        ds.close()
        ctx.close()
