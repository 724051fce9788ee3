"""Deep, degenerate and threshold-sized trees on the device.  Every tree the rest of the suite traverses is at most 16 levels deep; the builder
promises up to RTMI_BVH_STACK - 3 = 29, the trace kernels size their LDS stack columns from the scene's depth (choose_trace_kernel: depth + 2 rows,
the parked cursors and the camera-ray stash right behind them), and the chooser switches kernels on depth, node count, grid and primitive count.
The recipes of tests/tree_scenes.py put a scene on every side of every such switch; tests/test_tree_host.py pins their trees on the CPU, and every
test here first asserts DeviceScene.tree_info() against that table, so a builder that one day makes these trees shallow fails the test instead of
emptying it.  Each comparison is three-way: tree == flat scan bit for bit (NaN patterns included), and both == the CPU oracle's Hitlist."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from tests import tree_scenes as ts

FLT_MAX = 3.4028234663852886e38
RMS_TOL = 1e-4
UV_TOL_F32 = 6 * 2.0 ** -24
NX, NY, NS = 48, 32, 4
CHAINS = {7: (30, 0.9, 0.15), 14: (120, 0.9, 0.15), 26: (400, 0.9, 0.15), 29: (1000, 0.9, 0.15)}  # depth -> recipe, shallow first
CHAIN_F32 = (763, 0.95, 0.15)  # depth 27, every r * r a normal float
# what the f64 oracle answers for chain_rays(n, q, rho, 19700, 41) at t-min 0.001, t-max FLT_MAX: rays (of the 19 700 oblique ones) that end on
# the chain, distinct spheres among them.  t-min 0.001 hides the spheres smaller than that from the rays that start 1.5 radii away.
CHAIN_ORACLE = {7: (12020, 30), 14: (14017, 120), 26: (11003, 331), 29: (10164, 331)}


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _info_key(n, q, rho):
    return "chain(%d, %s, %s)" % (n, q, rho)


@functools.lru_cache(maxsize=None)
def _chain_flat(depth, lens=False, f32=False):
    n, q, rho = CHAIN_F32 if f32 else CHAINS[depth]
    return fl.flatten(ts.chain_scene(ts.chain(n, q, rho), lens))


@functools.lru_cache(maxsize=None)
def _oracle(precision):
    from oracle.oracle import Oracle
    return Oracle(precision)


@functools.lru_cache(maxsize=None)
def _chain_reference(depth):
    """the oracle's answers for a chain, computed once: hits under the three (t-min, t-max) pairs, the paths of every fifth ray"""
    n, q, rho = CHAINS[depth]
    f, orc = _chain_flat(depth), _oracle("f64")
    rays, n_fb = ts.chain_rays(n, q, rho, 19700, 41)
    hits = {tt: orc.probe_hit(f, rays, tmin=tt[0], tmax=tt[1]) for tt in ((0.001, FLT_MAX), (0.0, FLT_MAX), (0.001, 6.0))}
    sub = rays[::5]
    keys = np.random.default_rng(depth).integers(0, 2 ** 63, len(sub), dtype=np.uint64)
    paths = orc.probe_paths(f, sub, keys, depth=50, ctr0=0, max_seg=6)
    return rays, n_fb, hits, sub, keys, paths


def chain_oracle_stats(depth):
    """(oblique rays that end on the chain, distinct spheres they end on) by the oracle, default t range"""
    rays, n_fb, hits, _, _, _ = _chain_reference(depth)
    main = hits[(0.001, FLT_MAX)][:-n_fb]
    on_chain = (main[:, 0] == 1) & (main[:, 1] > 0)  # (primitive 0 is the dome)
    return int(on_chain.sum()), len(np.unique(main[on_chain, 1]))


def _open(f, info=None):
    ctx = core.Context(0)
    ds = core.DeviceScene(f, ctx=ctx)
    if info is not None:
        got = ds.tree_info()
        assert got == tuple(info), "the scene's tree is not the one this test is about: %r, expected %r" % (got, tuple(info))
    return ctx, ds


def _frame_matches_oracle(frame, exp, precision="f64", what=""):
    lin, q, cnt = frame
    exp_lin, exp_q, exp_cnt = exp
    if precision == "f64":  # the conditions of test_random_scenes_match_oracle
        assert np.array_equal(cnt, exp_cnt), (what, cnt, exp_cnt)
        err = rms(lin, exp_lin)
        assert err <= RMS_TOL and err < 1e-12, (what, err)
        assert np.abs(q.astype(int) - exp_q.astype(int)).max() <= 1, what
    else:  # ... and of test_f32_random_scenes_match_f32_oracle
        moved = int((np.abs(lin - exp_lin).max(axis=2) > 1e-5).sum())
        print("%s: f32 frame, pixels moved %d, segments %+d, rms %.3g" % (what, moved, int(cnt[0]) - int(exp_cnt[0]), rms(lin, exp_lin)))
        assert moved <= 2, (what, moved)
        assert abs(int(cnt[0]) - int(exp_cnt[0])) <= 102 and cnt[1] == exp_cnt[1], (what, cnt, exp_cnt)


def _hits_match_oracle(got, exp, precision="f64", what=""):
    assert _same(got[:, :9], exp[:, :9]), "%s: hit?, prim, t, p, normal must be bit-exact" % what
    hit = exp[:, 0] == 1
    if hit.any():
        err = float(np.nanmax(np.abs(got[hit, 9:11] - exp[hit, 9:11])))
        assert err <= (1e-14 if precision == "f64" else UV_TOL_F32), (what, err)


def _three_way(f, rays, info, precision="f64", ranges=((0.001, FLT_MAX),), frame=True, paths=0, suspend=(None,), what="", exp_hits=None):
    """tree == flat scan == oracle for probe_hit under every (t-min, t-max), optionally probe_paths of the first `paths` rays and a frame; the tree
    side once per suspend_lanes value.  -> the flat scan's hits under the first range"""
    orc = _oracle(precision)
    ctx, ds = _open(f, info)
    try:
        ctx.set_option("accel", 0)
        flat = {tt: ds.probe_hit(rays, tt[0], tt[1], precision=precision) for tt in ranges}
        for tt in ranges:
            exp = exp_hits[tt] if exp_hits is not None else orc.probe_hit(f, rays, tmin=tt[0], tmax=tt[1])
            _hits_match_oracle(flat[tt], exp, precision, "%s flat scan, t range %r" % (what, tt))
        if paths:
            keys = np.random.default_rng(len(rays)).integers(0, 2 ** 63, paths, dtype=np.uint64)
            p_flat = ds.probe_paths(rays[:paths], keys, depth=50, ctr0=0, max_seg=6, precision=precision)
            ergb, enseg, elog, enlog = orc.probe_paths(f, rays[:paths], keys, depth=50, ctr0=0, max_seg=6)
            if precision == "f64":
                assert np.array_equal(p_flat[1], enseg) and _same(p_flat[2], elog) and np.array_equal(p_flat[3], enlog), what + ": segment logs"
                assert np.allclose(p_flat[0], ergb, atol=1e-11, rtol=0, equal_nan=True)
            else:
                same = p_flat[1] == enseg
                assert same.mean() >= 0.999 and _same(p_flat[2][same], elog[same]), what + ": f32 segment logs"
                assert float(np.abs(p_flat[0][same] - ergb[same]).max()) <= 4e-6
        if frame:
            f_flat = ds.render(NX, NY, NS, precision=precision)
            assert ctx.last_accel() == "flat"
            _frame_matches_oracle(f_flat, orc.render(f, NX, NY, NS, 50, core.RENDER_SEED, nthreads=16), precision, what + " flat scan")
        ctx.set_option("accel", 1)
        for lanes in suspend:
            if lanes is not None:
                ctx.set_option("suspend_lanes", lanes)
            tag = "%s tree, suspend_lanes %r" % (what, lanes)
            for tt in ranges:
                assert _same(ds.probe_hit(rays, tt[0], tt[1], precision=precision), flat[tt]), "%s, t range %r: probe_hit" % (tag, tt)
            if paths:
                p_tree = ds.probe_paths(rays[:paths], keys, depth=50, ctr0=0, max_seg=6, precision=precision)
                assert all(_same(a, b) for a, b in zip(p_tree, p_flat)), tag + ": probe_paths"
            if frame:
                f_tree = ds.render(NX, NY, NS, precision=precision)
                assert ctx.last_accel() == "bvh", tag
                assert all(np.array_equal(a, b) for a, b in zip(f_tree, f_flat)), tag + ": frame and counters"
        return flat[ranges[0]]
    finally:
        ds.close()
        ctx.close()


# ---- 1. deep chain, probes -------------------------------------------------------------------------------------------------------------------
def test_chain_rays_reach_what_the_oracle_says():
    """the rays of the probe tests are not vacuous: by the oracle at least half of the oblique ones end on the chain, on at least 300 distinct
    spheres where the chain has that many (the exact figures of the committed, seeded rays are pinned)"""
    for depth in CHAINS:
        on_chain, distinct = chain_oracle_stats(depth)
        print("depth %d: %d of 19700 oblique rays end on the chain, %d distinct spheres" % (depth, on_chain, distinct))
        assert (on_chain, distinct) == CHAIN_ORACLE[depth]
        assert on_chain >= 19700 // 2 and distinct >= min(300, CHAINS[depth][0])


@pytest.mark.parametrize("node16", ["0", "1"])
@pytest.mark.parametrize("depth", list(CHAINS))
def test_deep_chain_probes(depth, node16, monkeypatch):
    """probe_hit and probe_paths down a chain of depth 7 / 14 / 26 / 29 (the builder's maximum), both node formats, t-min 0.001 and 0, t-max
    FLT_MAX and one that cuts the chain: half the rays descend the deep side first with every sibling box pushed"""
    monkeypatch.setenv("RTMI_NODE16", node16)
    n, q, rho = CHAINS[depth]
    rays, n_fb, hits, sub, keys, (ergb, enseg, elog, enlog) = _chain_reference(depth)
    f = _chain_flat(depth)
    flat = _three_way(f, rays, ts.HOST_TABLE[_info_key(n, q, rho)], ranges=tuple(hits), frame=False, suspend=(None,), what="depth %d node16 %s" % (depth, node16),
                      exp_hits=hits)
    main = flat[:-n_fb]
    on_chain = (main[:, 0] == 1) & (main[:, 1] > 0)
    assert (int(on_chain.sum()), len(np.unique(main[on_chain, 1]))) == CHAIN_ORACLE[depth]
    ctx, ds = _open(f)
    try:
        out = []
        for accel in (0, 1):
            ctx.set_option("accel", accel)
            out.append(ds.probe_paths(sub, keys, depth=50, ctr0=0, max_seg=6))
        assert all(_same(a, b) for a, b in zip(out[0], out[1])), "probe_paths: tree vs flat scan"
        assert np.array_equal(out[1][1], enseg) and _same(out[1][2], elog) and np.array_equal(out[1][3], enlog)
        assert np.allclose(out[1][0], ergb, atol=1e-11, rtol=0)
        assert enseg.max() >= 6 and enseg.mean() > 1.3
    finally:
        ds.close()
        ctx.close()


def test_deepest_chain_fills_the_stack():
    """count_traversal on a 16 x 16 x 1 frame of the depth-29 chain: more than 2 x 29 box tests per segment on average -- the rays do go down"""
    n, q, rho = CHAINS[29]
    ctx, ds = _open(_chain_flat(29), ts.HOST_TABLE[_info_key(n, q, rho)])
    try:
        ctx.set_option("count_traversal", 1)
        lin, _, cnt = ds.render(16, 16, 1)
        boxes, exact = ctx.last_traversal_counters()
        print("depth 29, 16 x 16 x 1: %d segments, %d box tests (%.1f per segment), %d exact tests" % (int(cnt[0]), boxes, boxes / float(cnt[0]), exact))
        assert boxes > 2 * 29 * int(cnt[0])
        ctx.set_option("count_traversal", 0)
        assert np.array_equal(ds.render(16, 16, 1)[0], lin)
    finally:
        ds.close()
        ctx.close()


# ---- 2. deep chain, renders: the stack columns sized per scene and the chooser's 40 KB switch ------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True])
@pytest.mark.parametrize("depth", list(CHAINS))
def test_deep_chain_renders(depth, lens):
    """pinhole (11 stash words: the LDS-stash kernel up to depth 21) and thin lens (17: up to depth 15), depths on both sides of both boundaries,
    time-sliced at 8 and 40 lanes and not at all: the frame of the tree is the frame of the flat scan and the oracle's"""
    n, q, rho = CHAINS[depth]
    f = _chain_flat(depth, lens)
    assert f.cam_kind == (1 if lens else 0)
    rays = ts.chain_rays(n, q, rho, 1700, 43)[0]
    _three_way(f, rays, ts.HOST_TABLE[_info_key(n, q, rho)], suspend=(0, 8, 40), what="depth %d lens %s" % (depth, lens))


def test_register_stash_kernel_on_a_tree_the_lds_stash_takes(monkeypatch):
    """RTMI_SPHERE_LDS_STASH=0 at depth 14: the register-stash instantiation (which the deep chains get anyway) gives the LDS-stash kernel's frame"""
    n, q, rho = CHAINS[14]
    frames = []
    for stash in (None, "0"):
        if stash is None:
            monkeypatch.delenv("RTMI_SPHERE_LDS_STASH", raising=False)
        else:
            monkeypatch.setenv("RTMI_SPHERE_LDS_STASH", stash)
        for lens in (False, True):
            ctx, ds = _open(_chain_flat(14, lens), ts.HOST_TABLE[_info_key(n, q, rho)])
            try:
                ctx.set_option("suspend_lanes", 8)
                frames.append(ds.render(NX, NY, NS))
                assert ctx.last_accel() == "bvh"
            finally:
                ds.close()
                ctx.close()
    for a, b in zip(frames[:2], frames[2:]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(frames[0][0], frames[1][0])  # (the two cameras do not see the same frame)


# ---- 3. deep chain, f32 ----------------------------------------------------------------------------------------------------------------------
def test_deep_chain_f32():
    """chain(763, 0.95, 0.15), depth 27, with the float kernels: tree == float flat scan bit for bit, both == the float oracle"""
    n, q, rho = CHAIN_F32
    f = _chain_flat(27, f32=True)
    rays = ts.chain_rays(n, q, rho, 19700, 41)[0]
    flat = _three_way(f, rays, ts.HOST_TABLE[_info_key(n, q, rho)], precision="f32", paths=4000, suspend=(None, 0), what="f32 depth 27")
    on_chain = (flat[:, 0] == 1) & (flat[:, 1] > 0)
    assert on_chain.mean() > 0.5 and len(np.unique(flat[on_chain, 1])) >= 250  # (the float oracle's: 0.58 and 290)


# ---- 4. deep mixed-kind tree -----------------------------------------------------------------------------------------------------------------
CHAIN_EXT = (400, 0.9, 0.15)
CHAIN_EXT_INFO = (499, 29, 0, 1)  # 501 primitives (320 spheres, 20 rectangles, 20 triangles, 20 boxes of six, 20 instanced spheres, the dome)


def test_deep_mixed_kind_tree():
    """the chain with every fifth item a rectangle / triangle / box / instanced sphere through the mixed-kind kernels (their stack columns are
    always sized from the depth, parked cursors right behind): tree == culled scan == the nested oracle, time-sliced and not"""
    from oracle.tree import flatten_with_tree
    n, q, rho = CHAIN_EXT
    f = flatten_with_tree(ts.chain_scene(ts.chain_ext(n, q, rho)))
    assert f.n_prims == 501
    rays = ts.chain_rays(n, q, rho, 7700, 43)[0]
    flat = _three_way(f, rays, CHAIN_EXT_INFO, paths=2000, suspend=(None, 0, 40), what="chain_ext")
    assert CHAIN_EXT_INFO[1] >= 26
    kinds = set((f.prim_kind[flat[flat[:, 0] == 1, 1].astype(int)] & 15).tolist())
    assert len(kinds) >= 5, kinds  # spheres, rectangles of two orientations at least, triangles ... are all among the hits


# ---- 5. exact ties through the tree ----------------------------------------------------------------------------------------------------------
def _tie_rays():
    rays = ts.cloud_rays(8000, 47, spread=1.0)
    d = np.random.default_rng(1).normal(0, 1, (200, 3))
    inside = np.concatenate([np.tile([1.5, 0.0, 0.0], (200, 1)), d, np.zeros((200, 1))], axis=1)
    return np.concatenate([rays, inside])


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("bystanders", [0, 12])
def test_identical_spheres_answer_the_first(bystanders, precision):
    """300 spheres of one centre and radius: every leaf ties exactly, and the Hitlist's answer -- the first -- must come out of the tree
    whatever order it visits them in (sphere_roots_any_order: the lowest index wins)"""
    name = "identical(300, 12)" if bystanders else "identical(300)"
    f = fl.flatten(ts.scene(ts.build(name)))
    flat = _three_way(f, _tie_rays(), ts.HOST_TABLE[name], precision=precision, suspend=(None, 0), what=name + " " + precision)
    tied = (flat[:, 0] == 1) & (flat[:, 1] < 300)
    assert tied.sum() > 2000 and (flat[tied, 1] == 0).all()


def test_concentric_shells_answer_the_outermost_from_outside_and_the_innermost_from_the_centre():
    f = fl.flatten(ts.scene(ts.build("shells(300)")))
    rng = np.random.default_rng(71)
    u = rng.normal(0, 1, (3000, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = np.array([1.5, 0.0, 0.0])
    outside = np.concatenate([c + 5.0 * u, -u + rng.normal(0, 0.02, (3000, 3)), np.zeros((3000, 1))], axis=1)
    centre = np.concatenate([np.tile(c, (3000, 1)), u, np.zeros((3000, 1))], axis=1)
    flat = _three_way(f, np.concatenate([outside, centre]), ts.HOST_TABLE["shells(300)"], suspend=(None, 0), what="shells")
    assert (flat[:3000, 0] == 1).all() and (flat[:3000, 1] == 299).all()
    assert (flat[3000:, 0] == 1).all() and (flat[3000:, 1] == 0).all() and np.allclose(flat[3000:, 2], 0.2, rtol=1e-12)


# ---- 6. more than 16 big primitives ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [False, True])
def test_more_big_primitives_than_the_cap(bvh):
    """twenty scene-sized shells: sixteen are tested exactly for every ray, the innermost four -- among them the light -- sit in the tree with
    boxes the size of the scene.  Rays start between the shells and inside the cloud."""
    f = fl.flatten(ts.scene(ts.many_big(20, 300), bvh=bvh))
    rng = np.random.default_rng(59)
    u = rng.normal(0, 1, (4000, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    between = np.concatenate([u * rng.uniform(40.0, 60.0, (4000, 1)), rng.normal(0, 1, (4000, 3)), np.zeros((4000, 1))], axis=1)
    flat = _three_way(f, np.concatenate([between, ts.cloud_rays(4000, 61)]), ts.HOST_TABLE["many_big(20, 300)"], paths=2000, suspend=(None, 0),
                      what="many_big bvh %s" % bvh)
    prim = flat[flat[:, 0] == 1, 1]
    assert (flat[:, 0] == 1).all() and ((prim >= 16) & (prim < 20)).sum() > 500 and (prim < 16).sum() > 500 and (prim >= 20).sum() > 500


# ---- 7. negative and zero radius -------------------------------------------------------------------------------------------------------------
def _scan_variants(ctx):
    ok = []
    for v in range(8):
        try:
            ctx.set_option("scan_variant", v)
        except core.RtmiError:
            continue
        ok.append(v)
    return ok


@pytest.mark.parametrize("name", ["negative_radius(200)", "zero_radius(200)"])
def test_negative_and_zero_radius(name):
    """prim_world_box takes |r|; the exact test squares r; the hit record's normal is normalise(p - centre) (hitable.clj:194), which does not see
    the radius' sign -- so a sphere of radius -r is the sphere of radius r, outward normal included, in the tree, in every scan variant (LDS
    and scalar, cull on and off) and in the oracle.  Radius 0: rays aimed at the centres exactly, NaN patterns compared as they come."""
    f = fl.flatten(ts.scene(ts.build(name)))
    rays = ts.cloud_rays(12000, 53)
    if name.startswith("zero"):
        c = f.prim_geom[1:201, :3]
        o = np.array(ts.CAMERA_AT) + np.random.default_rng(2).normal(0, 1, (200, 3))
        rays = np.concatenate([rays, np.concatenate([o, c - o, np.zeros((200, 1))], axis=1), np.concatenate([o, (c - o) * 0.5, np.zeros((200, 1))], axis=1)])
    flat = _three_way(f, rays, ts.HOST_TABLE[name], ranges=((0.001, FLT_MAX), (0.0, FLT_MAX)), paths=4000, suspend=(None, 0), what=name)
    hit = flat[:, 0] == 1
    idx = flat[hit, 1].astype(int)
    rad = f.prim_geom[idx, 3]
    if name.startswith("negative"):
        out = np.einsum("ij,ij->i", flat[hit, 6:9], flat[hit, 3:6] - f.prim_geom[idx, :3])
        assert (rad < 0).sum() > 1000 and (out[rad < 0] > 0).all()
    else:
        assert (rad == 0).sum() >= 100  # (the oracle's count for these rays: 396)
    ctx, ds = _open(f)
    try:
        ctx.set_option("accel", 0)
        variants = _scan_variants(ctx)
        assert len(variants) >= 4, variants
        first = None
        for v in variants:
            ctx.set_option("scan_variant", v)
            got = (ds.probe_hit(rays), ds.probe_hit(rays, 0.0, FLT_MAX), ds.render(NX, NY, NS))
            first = first or got
            assert _same(got[0], flat) and _same(got[1], first[1]), "scan_variant %d: probe_hit" % v
            assert all(np.array_equal(a, b) for a, b in zip(got[2], first[2])), "scan_variant %d: frame" % v
    finally:
        ds.close()
        ctx.close()


# ---- 8. the chooser's thresholds, both sides -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cloud(128)", "cloud(129)", "layer(255)", "layer(256)"])
def test_sphere_kernel_thresholds(name):
    """127 / 128 inner nodes: the plain and the time-sliced instantiation; 255 / 256 layer primitives: without and with the entry grid"""
    f = fl.flatten(ts.scene(ts.build(name)))
    rays = ts.cloud_rays(8000, 67)
    if name.startswith("layer"):  # rays that graze along the layer, crossing many grid cells
        rng = np.random.default_rng(73)
        o = np.stack([rng.uniform(-12, 12, 4000), rng.uniform(0.0, 0.6, 4000), rng.uniform(-12, 12, 4000)], axis=1)
        d = np.stack([rng.normal(0, 1, 4000), rng.normal(0, 0.03, 4000), rng.normal(0, 1, 4000)], axis=1)
        rays = np.concatenate([rays, np.concatenate([o, d, np.zeros((4000, 1))], axis=1)])
    info = ts.HOST_TABLE[name]
    sliced, grid = {"cloud(128)": (False, False), "cloud(129)": (True, False), "layer(255)": (True, False), "layer(256)": (True, True)}[name]
    assert (info[0] >= 128) == sliced and (info[2] > 0) == grid  # what the chooser will decide from
    flat = _three_way(f, rays, info, paths=2000, suspend=(None, 0), what=name)
    assert len(np.unique(flat[flat[:, 0] == 1, 1])) > 100


MIXED_INFO = {64: (62, 9, 0, 1), 65: (63, 7, 0, 1)}  # (the dome is the big primitive; n - 2 inner nodes over the other n - 1)


@pytest.mark.parametrize("n", [64, 65])
def test_small_world_scan_threshold(n, monkeypatch):
    """a mixed-kind Hitlist of exactly 64 primitives takes the small-world scan, one of 65 the culled scan: both == the tree == the nested oracle;
    last_accel says which of tree and scan ran"""
    from oracle.tree import flatten_with_tree
    f = flatten_with_tree(ts.scene(ts.mixed(n)))
    assert f.n_prims == n
    rays = ts.cloud_rays(8000, 67)
    flat = _three_way(f, rays, MIXED_INFO[n], paths=2000, suspend=(None,), what="mixed(%d)" % n)
    assert len(np.unique(flat[flat[:, 0] == 1, 1])) >= 60
    monkeypatch.setenv("RTMI_SMALL_SCAN", "0")  # read at scene creation: the culled scan at both sizes
    ctx, ds = _open(f)
    try:
        ctx.set_option("accel", 0)
        assert _same(ds.probe_hit(rays), flat)
        culled = ds.render(NX, NY, NS)
        assert ctx.last_accel() == "flat"
    finally:
        ds.close()
        ctx.close()
    monkeypatch.delenv("RTMI_SMALL_SCAN")
    ctx, ds = _open(f)
    try:
        frame = ds.render(NX, NY, NS)  # the library's default: the tree (the suite switches the shortcut for small mixed-kind scenes off)
        assert ctx.last_accel() == "bvh" and all(np.array_equal(a, b) for a, b in zip(frame, culled))
        ctx.set_option("flat_below", 1000)
        monkeypatch.delenv("RTMI_FLAT_BELOW", raising=False)
        again = ds.render(NX, NY, NS)  # with the shortcut: a request for the tree answered with the scan
        assert ctx.last_accel() == "flat" and all(np.array_equal(a, b) for a, b in zip(again, culled))
    finally:
        ds.close()
        ctx.close()
