"""The ray depth limit and the seed in whole frames, through every trace kernel the library can launch.

Every other frame of the suite is rendered at depth 50, where the per-lane depth counter of trace_kernel is almost never read: a lane whose counter lost or
gained a few units -- a parked passenger decremented by the shading, a stash entry dealt without its depth, a refill that forgets it -- renders the same
frame.  At depths 0 .. 3 the counter ends most paths (test_depth_reference.py holds the floors: >= 10 % of the paths end at the limit, neighbouring limits
differ by >= 1000 segments and >= 1e-3 rms), lanes die at the limit while their neighbours go on, and are refilled next to lanes parked inside the tree.

  * frames at depths 0, 1, 2, 3, 7 (and 1000 on the cover scene) against oracle.render, through every way of selecting a kernel a scene admits, all of
    them bit-identical among themselves;
  * probe_paths at those depths against the prefix rule (depth_cases.py) over the device's own depth-50 paths, and whole frames against the device's own
    depth-50 samples;
  * the other entry points (progressive, adaptive, region, multi, dealt tiles) at depth 2;
  * 64-bit seeds that differ in their high bits, their sign bit, or everywhere.

Tolerances are those of the depth-50 tests of the same scenes with the depth written in (depth_cases.check_*)."""
import contextlib
import os

import numpy as np
import pytest

import depth_cases as dc
import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl

pytestmark = pytest.mark.gpu

WHOLE_LDS = 64 * 1024 - 64   # option lds_tile_bytes as a context starts with it


class Family:
    """one way of selecting a trace kernel: environment read when the scene is created, environment read at the launch, context options, and what
    rtmi_last_accel must say afterwards"""

    def __init__(self, tag, runs, create_env=None, launch_env=None, **options):
        self.tag, self.runs, self.create_env, self.launch_env, self.options = tag, runs, create_env or {}, launch_env or {}, options


def _sphere_families():
    """choose_trace_kernel for a world of spheres.  The cover scene's tree has an entry grid, and a scene with a grid always runs a time-sliced
    instantiation (suspend_lanes = 0 is then the threshold 0): RTMI_GRID=0 reaches the instantiations without the slicing machinery."""
    fams = [Family("flat scan, variant %d" % v, "flat", accel=0, scan_variant=v) for v in range(4)]
    fams += [Family("flat scan, variant %d, 1 KiB LDS tiles%s" % (v, " (MULTI)" if v < 2 else ""), "flat", accel=0, scan_variant=v, lds_tile_bytes=1024) for v in range(4)]
    fams += [Family("tree, time-sliced, LDS stash", "bvh"),
             Family("tree, time-sliced, register stash", "bvh", launch_env={"RTMI_SPHERE_LDS_STASH": "0"}),
             Family("tree, suspend_lanes 0", "bvh", suspend_lanes=0),
             Family("tree, suspend_lanes 64", "bvh", suspend_lanes=64),
             Family("tree, counting", "bvh", count_traversal=1),
             Family("tree, 64-byte nodes", "bvh", create_env={"RTMI_NODE16": "0"}),
             Family("tree, 32-byte nodes", "bvh", create_env={"RTMI_NODE16": "1"}),
             Family("tree, no grid, unsliced", "bvh", create_env={"RTMI_GRID": "0"}, suspend_lanes=0),
             Family("tree, no grid, unsliced, counting", "bvh", create_env={"RTMI_GRID": "0"}, suspend_lanes=0, count_traversal=1)]
    return fams


def _mixed_families():
    return [Family("small-world scan", "flat", accel=0),
            Family("culled scan", "flat", create_env={"RTMI_SMALL_SCAN": "0"}, accel=0),
            Family("tree, suspend_lanes 12", "bvh", suspend_lanes=12),
            Family("tree, suspend_lanes 0", "bvh", suspend_lanes=0),
            Family("tree, counting", "bvh", count_traversal=1),
            Family("tree, boxes as six leaves", "bvh", create_env={"RTMI_BOX_LEAF": "0"}),
            Family("tree, boxes as one leaf", "bvh", create_env={"RTMI_BOX_LEAF": "1"})]


def _media_families():
    return [Family("flat", "flat", accel=0), Family("tree", "bvh"), Family("tree, counting", "bvh", count_traversal=1)]


FAMILIES = {"sphere": _sphere_families(), "mixed": _mixed_families(), "media": _media_families()}
DEFAULTS = {"accel": 1, "scan_variant": 3, "lds_tile_bytes": WHOLE_LDS, "count_traversal": 0, "flat_below": 0}
SUSPEND = {"sphere": 8, "mixed": 12, "media": 12}   # what a launch takes when the host never set the option


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def device():
    """(scene name or FlatScene, creation environment) -> (context, device scene), made once for the module"""
    made = {}

    def get(scene, create_env=None):
        env = create_env or {}
        key = (scene if isinstance(scene, str) else id(scene), tuple(sorted(env.items())))
        if key not in made:
            with _environ(env):
                ctx = core.Context(0)
                made[key] = (ctx, core.DeviceScene(dc.flat(scene) if isinstance(scene, str) else scene, ctx=ctx))
        return made[key]

    yield get
    for ctx, ds in made.values():
        ds.close()
        ctx.close()


def _set_options(ctx, kind, **options):
    """every option a family may touch: the defaults of a fresh context, then the family's own"""
    every = dict(DEFAULTS, suspend_lanes=SUSPEND[kind])
    every.update(options)
    for k, v in every.items():
        ctx.set_option(k, v)


def _render(device, name, fam, shape, d, precision="f64", seed=dc.SEED, scene=None):
    kind = dc.SCENES[name][2]
    ctx, ds = device(scene if scene is not None else name, fam.create_env)
    _set_options(ctx, kind, **fam.options)
    nx, ny, ns = shape
    with _environ(fam.launch_env):
        out = ds.render(nx, ny, ns, depth=d, seed=seed, precision=precision)
    assert ctx.last_accel() == fam.runs, (name, fam.tag, "rtmi_last_accel says %s" % ctx.last_accel())
    return out


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


# ---- 1. frames against the oracle: every kernel family, every depth -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,d", dc.frame_cases(), ids=["%s-%dx%dx%d-depth%d" % ((n,) + s + (d,)) for n, s, d in dc.frame_cases()])
def test_frames_at_every_depth_through_every_kernel_family(request, device, name, shape, d):
    kind, exact = dc.SCENES[name][2], dc.SCENES[name][3]
    for precision in (("f64", "f32") if kind == "sphere" else ("f64",)):
        exp = dc.oracle_frame(_oracle(request, precision), name, shape, d)
        first = None
        for fam in FAMILIES[kind]:
            what = "%s %dx%dx%d depth %d %s: %s" % ((name,) + shape + (d, precision, fam.tag))
            got = _render(device, name, fam, shape, d, precision)
            print("%s: total-rays %d (oracle %+d), rms %.3g, %d pixels beyond 1e-9" % (what, int(got[2][0]), int(got[2][0]) - int(exp[2][0]), dc.rms(got[0], exp[0]),
                                                                                      int((np.abs(got[0] - exp[0]).max(axis=2) > 1e-9).sum())))
            if precision == "f32":
                dc.check_frame_f32(got, exp, d, what)
            elif exact:
                dc.check_frame_f64(got, exp, what)
            else:
                dc.check_frame_media(got, exp, d, what)
            if d == 0:
                assert int(got[2][0]) == shape[0] * shape[1] * shape[2] and int(got[2][1]) == shape[0] * shape[1], (what, "depth 0: one segment per sample", list(got[2]))
            if first is None:
                first = (fam.tag, got)
            else:
                for part, a, b in zip(("linear", "rgb8", "counters"), got, first[1]):
                    assert np.array_equal(a, b), (what, "%s differs from the family '%s'" % (part, first[0]))


def test_the_families_select_what_they_say(device):
    """what the launch decisions are taken from: the cover scene's tree is large enough to be time-sliced and has an entry grid unless RTMI_GRID=0; make-final's
    tree is time-sliced, the Cornell box's (fewer than 128 node records) never is; the node format follows RTMI_NODE16"""
    nodes, _, grid, _ = device("cover")[1].tree_info()
    assert nodes >= 128 and grid > 0
    assert device("cover", {"RTMI_GRID": "0"})[1].tree_info()[2] == 0 and device("cover", {"RTMI_GRID": "0"})[1].tree_info()[0] >= 128
    assert device("final")[1].tree_info()[0] >= 128 > device("cornell")[1].tree_info()[0] > 0
    print("node records: cover %d (grid %d), final %d, cornell %d" % (nodes, grid, device("final")[1].tree_info()[0], device("cornell")[1].tree_info()[0]))


# ---- 2. paths against the prefix rule, on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.SCENES))
def test_device_paths_are_the_prefix_of_their_depth_50_selves(oracle, device, name):
    """ds.probe_paths at every depth against prefix_expectation of the device's OWN depth-50 run of the same rays, flat scan and tree: bit for bit on the
    sphere and rectangle worlds, test_media_match_oracle's rule for paths where media are"""
    exact = dc.SCENES[name][3]
    rays, keys, ctr0 = dc.camera_paths(oracle, name)
    ctx, ds = device(name)
    try:
        for accel in (0, 1):
            ctx.set_option("accel", accel)
            rgb50, nseg50, log50, _ = ds.probe_paths(rays, keys, depth=dc.FULL, ctr0=ctr0, max_seg=dc.LOG50)
            for d in dc.DEPTHS:
                got = ds.probe_paths(rays, keys, depth=d, ctr0=ctr0, max_seg=dc.max_seg(d))
                dc.check_paths(got, dc.prefix_expectation(rgb50, nseg50, log50, d), exact, (name, "accel", accel, "depth", d))
                assert got[1].max() == d + 1 and (d > 3 or dc.limit_share(nseg50, d) >= 0.1)  # (the floor of test_depth_reference.py, on the device's own paths)
    finally:
        ctx.set_option("accel", 1)


def test_frames_against_the_device_own_depth_50_samples(device):
    """A 16 x 8 x 2 frame of the cover scene, every sample probed on its own at depth 50 with the key the frame gives it (depth_cases.frame_paths): the
    samples fold to the depth-50 frame; the frame at depth d equals the depth-50 frame in every pixel whose paths all have at most d + 1 segments -- and
    everywhere the frame of the prefix rule's colours, with the rule's segments as total-rays"""
    nx, ny, ns = 16, 8, 2
    ctx, ds = device("cover")
    try:
        for accel in (0, 1):
            ctx.set_option("accel", accel)
            rays, keys, ctr = dc.frame_paths(ds.probe_camera, ds.flat, nx, ny, ns)
            rgb50, nseg50, log50, _ = dc.probe_frame_paths(ds.probe_paths, rays, keys, ctr, dc.FULL, dc.LOG50)
            f50 = ds.render(nx, ny, ns, depth=dc.FULL)
            assert np.array_equal(dc.frame_of(rgb50, nx, ny, ns), f50[0]) and int(nseg50.sum()) == int(f50[2][0]), accel
            for d in dc.DEPTHS:
                lin, q, cnt = ds.render(nx, ny, ns, depth=d)
                short = dc.pixel_image(nseg50 <= d + 1, nx, ny, ns).all(axis=2)
                assert 0 < short.sum() and (short.sum() < nx * ny or d == 7), (accel, d, int(short.sum()))
                assert np.array_equal(lin[short], f50[0][short]) and np.array_equal(q[short], f50[1][short]), (accel, d)
                rgb, nseg, _, _ = dc.prefix_expectation(rgb50, nseg50, log50, d)
                assert np.array_equal(lin, dc.frame_of(rgb, nx, ny, ns)) and int(cnt[0]) == int(nseg.sum()), (accel, d)
    finally:
        ctx.set_option("accel", 1)


# ---- 3. the other entry points carry the depth -----------------------------------------------------------------------------------------------
CHUNKS = (1, 3, 4)


@pytest.fixture(scope="module")
def cover_depth_2_and_3(device):
    """one-shot frames of the cover scene's two shapes at depths 2 and 3 with k = 1, 4, 8 samples (the ends of CHUNKS) and the shape's own count"""
    ctx, ds = device("cover")
    _set_options(ctx, "sphere")
    out = {}
    for nx, ny, ns in dc.SCENES["cover"][1]:
        for k in sorted(set(np.cumsum(CHUNKS).tolist() + [ns])):
            for d in (2, 3):
                out[(nx, ny, k, d)] = ds.render(nx, ny, k, depth=d)
    return out


@pytest.mark.parametrize("shape", dc.SCENES["cover"][1], ids=lambda s: "%dx%dx%d" % s)
def test_progressive_and_adaptive_frames_carry_the_depth(device, cover_depth_2_and_3, shape):
    nx, ny, _ = shape
    ctx, ds = device("cover")
    try:
        k = 0
        for n in CHUNKS:
            lin, q, err, cnt = ds.render_progressive(nx, ny, k, n, depth=2)
            k += n
            assert dc.frames_equal((lin, q, cnt), cover_depth_2_and_3[(nx, ny, k, 2)]), ("progressive", k)
            assert not np.array_equal(lin, cover_depth_2_and_3[(nx, ny, k, 3)][0]) and int(cnt[0]) < int(cover_depth_2_and_3[(nx, ny, k, 3)][2][0])
        with pytest.raises(core.RtmiError):  # the frame was started at depth 2
            ds.render_progressive(nx, ny, k, 1, depth=3)
        ctx.progressive_release()
        k = 0
        for n in CHUNKS:
            lin, q, err, smp, cnt = ds.render_adaptive(nx, ny, k, n, 0.0, depth=2)
            k += n
            for held in np.unique(smp):  # (eps = 0 retires only a tile whose samples are all equal: it then holds fewer samples, and is that frame's tile)
                ref = cover_depth_2_and_3[(nx, ny, int(held), 2)]
                assert np.array_equal(lin[smp == held], ref[0][smp == held]) and np.array_equal(q[smp == held], ref[1][smp == held]), ("adaptive", k, held)
            assert (smp == k).mean() > 0.9
            if (smp == k).all():
                assert np.array_equal(cnt, cover_depth_2_and_3[(nx, ny, k, 2)][2]), ("adaptive", k)
    finally:
        ctx.progressive_release()


@pytest.mark.parametrize("shape", dc.SCENES["cover"][1], ids=lambda s: "%dx%dx%d" % s)
def test_region_multi_and_dealt_tiles_carry_the_depth(device, cover_depth_2_and_3, shape):
    import torch
    from raytrace_clj_amd import dist as rdist
    nx, ny, ns = shape
    ctx, ds = device("cover")
    _set_options(ctx, "sphere")
    whole = cover_depth_2_and_3[(nx, ny, ns, 2)]
    deeper = cover_depth_2_and_3[(nx, ny, ns, 3)]
    assert not np.array_equal(whole[0], deeper[0]) and int(whole[2][0]) + 1000 <= int(deeper[2][0])
    x0, y0, x1, y1 = 5, 3, 50, 30
    part, qp, cp = ds.render(nx, ny, ns, depth=2, region=(x0, y0, x1, y1))
    assert np.array_equal(part, whole[0][y0:y1, x0:x1]) and np.array_equal(qp, whole[1][y0:y1, x0:x1]) and int(cp[1]) == (x1 - x0) * (y1 - y0)
    md = rdist.MultiDevice(ds.flat, [0, 0])  # rtmi_render_multi, two replicas on device 0
    try:
        assert dc.frames_equal(md.render(nx, ny, ns, depth=2), whole), "rtmi_render_multi"
        k = 0
        for n in CHUNKS:
            lin, q, err, cnt = md.render_progressive(nx, ny, k, n, depth=2)
            k += n
            assert dc.frames_equal((lin, q, cnt), cover_depth_2_and_3[(nx, ny, k, 2)]), ("MultiDevice.render_progressive", k)
        md.progressive_release()
    finally:
        md.close()
    tr = rdist.TileRenderer(ds, nx, ny, 0, 1)  # rtmi_render_tiles_device + rtmi_assemble_device
    tr.step(ns, depth=2)
    torch.cuda.synchronize()
    assert np.array_equal(tr.linear.cpu().numpy(), whole[0]) and np.array_equal(tr.rgb8.cpu().numpy(), whole[1])
    assert [int(v) for v in tr.counters.cpu()] == [int(whole[2][0]), nx * ny]
    # ... and dealt over three ranks: every rank's tiles are the frame's, the ranks' segments add up
    world, tiles_x, rays = 3, (nx + 7) // 8, 0
    for rank in range(world):
        local = torch.zeros((rdist.tiles_per_rank(nx, ny, world), 64, 3), dtype=torch.float64, device="cuda")
        counters = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ds.render_tiles_device(nx, ny, ns, rank, world, local, counters, depth=2)
        torch.cuda.synchronize()
        rays += int(counters[0])
        local = local.cpu().numpy()
        for k, g in enumerate(rdist.local_tile_ids(nx, ny, rank, world)):
            ty, tx = (g // tiles_x) * 8, (g % tiles_x) * 8
            tile = local[k].reshape(8, 8, 3)[:min(8, ny - ty), :min(8, nx - tx)]
            assert np.array_equal(tile, whole[0][ty:ty + 8, tx:tx + 8]), (rank, g)
    assert rays == int(whole[2][0])


# ---- 4. seeds ------------------------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0xFEDCBA9876543210)
SEED_SHAPE = (24, 16, 2)


@pytest.fixture(scope="module")
def seed_scene():
    return fl.flatten(r.scene.make_random_scene(24, 16, 3, False))


@pytest.mark.parametrize("d", [dc.FULL, 2])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_seeds_of_64_bits_reach_the_kernels_whole(request, device, seed_scene, precision, d):
    """a seed truncated to 32 bits, sign-extended or halved on its way through the binding, TraceParams or the stream key would render another seed's frame:
    each seed against the oracle under the rules of the frames above, flat scan and tree, and no two seeds the same frame"""
    o = _oracle(request, precision)
    nx, ny, ns = SEED_SHAPE
    frames = {}
    for seed in SEEDS:
        exp = o.render(seed_scene, nx, ny, ns, d, seed, nthreads=4)
        for fam in (Family("flat scan", "flat", accel=0), Family("tree", "bvh")):
            what = "seed %#x depth %d %s: %s" % (seed, d, precision, fam.tag)
            got = _render(device, "cover", fam, SEED_SHAPE, d, precision, seed=seed, scene=seed_scene)
            if precision == "f32":
                dc.check_frame_f32(got, exp, d, what)
            else:
                dc.check_frame_f64(got, exp, what)
            assert dc.frames_equal(got, frames.setdefault(seed, got)), (what, "flat scan and tree differ")
    for a in SEEDS:
        for b in SEEDS:
            if a < b:
                assert not np.array_equal(frames[a][0], frames[b][0]), "seeds %#x and %#x render the same frame" % (a, b)


def test_progressive_frame_refuses_a_seed_that_differs_in_bit_63(device, seed_scene):
    nx, ny, _ = SEED_SHAPE
    ctx, ds = device(seed_scene)
    try:
        for seed in (1, 0xFEDCBA9876543210):
            first = ds.render_progressive(nx, ny, 0, 1, depth=2, seed=seed)
            with pytest.raises(core.RtmiError):
                ds.render_progressive(nx, ny, 1, 1, depth=2, seed=seed ^ (1 << 63))
            with pytest.raises(core.RtmiError):
                ds.render_progressive(nx, ny, 1, 1, depth=2, seed=seed ^ (1 << 32))
            lin, q, err, cnt = ds.render_progressive(nx, ny, 1, 1, depth=2, seed=seed)  # the frame is still there, under its own seed
            assert dc.frames_equal((lin, q, cnt), ds.render(nx, ny, 2, depth=2, seed=seed)) and not np.array_equal(lin, first[0])
            ctx.progressive_release()
    finally:
        ctx.progressive_release()
