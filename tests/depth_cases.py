"""Shared by test_depth_reference.py (CPU) and test_gpu_depth.py (GPU): the scenes, frame shapes and depth limits at which the ray depth limit
of core.clj:17-41 decides most samples, and the prefix rule -- a numpy statement of what a path at depth d is, given the same path at depth 50,
that never goes through anybody's `depth` argument.  Nothing here imports the device library; the oracle is passed in.  Not a test module
(pytest collects test_*.py only).

The prefix rule.  The random stream of a path is a function of (seed, pixel, sample) only, and `color` (core.clj:25-41) asks
(and (pos? depth) (scatter ...)) AFTER the hit test of a segment: a path at depth d walks the first d + 1 segments of its depth-50 self, hit for
hit and draw for draw.  If the depth-50 path has at most d + 1 segments, nothing differs.  If it has more, the hit of segment d + 1 scattered at
depth 50 -- so its material is no light and emits (0, 0, 0) --, every hit before it scattered as well, and the path at depth d ends there with
`scatter` never called: colour exactly (0, 0, 0), d + 1 segments, the segment's log record without a scattered direction."""
import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import flatten as fl

SEED = 0x5EED0002          # core.RENDER_SEED
DEPTHS = (0, 1, 2, 3, 7)   # limits at which the per-lane depth counter decides most samples ...
FULL = 50                  # ... the limit every other frame of the suite uses ...
DEEP = 1000                # ... and one no path of the cover scene reaches: the unlimited frame (cover only)
N_PATHS = 8192             # camera paths per scene for the probes
LOG50 = 12                 # segments logged of a depth-50 path: every max_seg(d) below fits


def max_seg(d):
    return min(d + 1, LOG50)


def _hitlist_media(nx, ny):
    from tests.test_gpu_round3 import hitlist_media_scene      # the MSEQ = 1 world: a Hitlist holding media
    return hitlist_media_scene()


def _narrowed_media(nx, ny):
    from tests.test_gpu_round4 import narrowed_media_scene     # the MSEQ = 2 world: Hitlists holding media below bvh-nodes
    return narrowed_media_scene()


# name -> (scene function, frame shapes (nx, ny, ns), kind, bit-exact against the oracle?).  A scene is made for its FIRST shape; the cover scene's second
# shape has partial 8x8 tiles, so items outside the image share waves with lanes cut at the limit (61 x 37 x 5 tells depth 3 from depth 4 by 801 segments
# only, x 6 by 976, x 7 by 1133: seven samples, so that test_depth_reference.py's floor of 1000 holds for it too).  kind: "sphere" worlds run the sphere kernels (both
# precisions), "mixed" the mixed-kind ones, "media" the Hitlist-with-media ones.  Paths through a ConstantMedium pass through log (ocml vs glibc): the
# media rule (check_paths, check_frame_media) instead of bit equality.
SCENES = {
    "cover": (lambda nx, ny: r.scene.make_random_scene(nx, ny, 11, True), ((64, 32, 8), (61, 37, 7)), "sphere", True),
    "cornell": (r.scene.make_cornell_box, ((48, 48, 8),), "mixed", True),
    "final": (r.scene.make_final, ((48, 48, 4),), "mixed", False),
    "hitlist-media": (_hitlist_media, ((64, 32, 8),), "media", False),
    "narrowed-media": (_narrowed_media, ((64, 32, 8),), "media", False),
}
MSEQ = {"hitlist-media": 1, "narrowed-media": 2}


def depths(name):
    return DEPTHS + ((DEEP,) if name == "cover" else ())


def frame_cases():
    """every (scene, (nx, ny, ns), depth) the GPU file renders; depth 1000 on the cover scene's first shape only"""
    return [(name, shape, d) for name, (_, shapes, _, _) in SCENES.items() for shape in shapes for d in depths(name)
            if d != DEEP or shape == shapes[0]]


_flat, _frames, _paths = {}, {}, {}


def flat(name):
    """the scene flattened, with its nested world for the oracle where the world is more than spheres"""
    if name not in _flat:
        make, shapes, kind, _ = SCENES[name]
        sc = make(*shapes[0][:2])
        if kind == "sphere":
            _flat[name] = fl.flatten(sc)
        else:
            from oracle.tree import flatten_with_tree
            _flat[name] = flatten_with_tree(sc)
    return _flat[name]


def oracle_frame(oracle, name, shape, d, seed=SEED):
    """oracle.render of a scene at one shape and depth, computed once per precision -> (linear, rgb8, counters); do not write into it"""
    key = (oracle.precision, name, shape, d, seed)
    if key not in _frames:
        nx, ny, ns = shape
        _frames[key] = oracle.render(flat(name), nx, ny, ns, d, seed, nthreads=16)
    return _frames[key]


def camera_paths(oracle, name, n=N_PATHS):
    """n camera rays of a scene with their stream keys -> (rays [n, 7], keys, ctr0: the draw at which every path starts), once per scene"""
    key = (oracle.precision, name, n)
    if key not in _paths:
        rng = np.random.default_rng(2)
        keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
        cam = oracle.probe_camera(flat(name), rng.random((n, 2)), keys)
        _paths[key] = (np.ascontiguousarray(cam[:, :7]), keys, int(cam[:, 7].max()))
    return _paths[key]


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


# ---- the prefix rule ----------------------------------------------------------------------------------------------------------------------
def prefix_expectation(rgb50, nseg50, log50, d):
    """What probe_paths(depth = d, max_seg = max_seg(d)) must return, from the SAME rays' probe_paths(depth = 50, max_seg >= max_seg(d)):
    -> (rgb [n, 3], nseg [n], log [n, max_seg(d), 12], nlog [n]).  core.clj:25-41 restated, for d < 50:
      nseg_d = min(nseg50, d + 1);
      rgb_d = rgb50 where nseg50 <= d + 1, else exactly (0, 0, 0);
      the logged records are the first max_seg(d) of the depth-50 log that fall inside the first nseg_d segments, and a cut path's last record has its
      scattered direction and its scattered? flag (fields 8..11) zero.
    A record is a HIT (a segment that misses everything is counted and not logged, so only a path's last segment can lack one); t > t-min > 0 marks
    the records the depth-50 log holds."""
    assert 0 <= d < FULL and log50.shape[1] >= max_seg(d) and log50.shape[2] == 12
    nseg50 = np.asarray(nseg50, np.int64)
    cut = nseg50 > d + 1
    nseg = np.minimum(nseg50, d + 1).astype(np.uint64)
    rgb = np.where(cut[:, None], 0.0, rgb50)
    m = max_seg(d)
    held = log50[:, :m, 1] != 0                    # records the depth-50 log holds among its first m
    assert (held[:, 1:] <= held[:, :-1]).all()     # (a log is a prefix: no holes)
    inside = np.arange(m)[None, :] < np.minimum(nseg50, d + 1)[:, None]
    keep = held & inside
    log = np.where(keep[:, :, None], log50[:, :m], 0.0)
    if m == d + 1:                                 # (the cut segment itself is logged only if the log is long enough to reach it)
        log[cut, d, 8:12] = 0.0
    assert keep[cut].all()                         # every segment of a path that went on past d + 1 was a hit
    return rgb, nseg, log, keep.sum(axis=1).astype(np.int32)


def limit_share(nseg50, d):
    """share of the paths that end at the limit d: their last segment is number d + 1, the one traced with the depth counter at 0 (nseg_d == d + 1)"""
    return float((np.asarray(nseg50, np.int64) >= d + 1).mean())


def cut_share(nseg50, d):
    """share of the paths the limit d changes: cut at segment d + 1 with more to come at depth 50 (nseg50 > d + 1)"""
    return float((np.asarray(nseg50, np.int64) > d + 1).mean())


# ---- every sample of a frame on its own, from the probes ------------------------------------------------------------------------------------
def frame_paths(probe_camera, f, nx, ny, ns, seed=SEED):
    """pixel() of rt_oracle.c (core.clj:43-51) up to the camera ray, for every sample of an nx x ny x ns frame in FP64: -> (rays [n, 7], keys [n], ctr [n] = the
    draw at which the sample's path starts), n = nx ny ns in [i, j, s] order, reference coordinates (j = 0 at the bottom).  probe_camera(uv, keys) -> [n, 8]
    is the oracle's or the device's.  u = (i + draw 0) / nx, v = (j + draw 1) / ny; a pinhole camera draws nothing more.  A thin lens draws its disk point
    from draw 2 on (a rejection loop) and then the ray's time, while the probe starts its stream at draw 0 -- but with aperture 0 the disk point is
    multiplied by 0, so origin and direction are the probe's whatever it drew, and the loop and the time are restated here."""
    import frame_reference as fr
    ii, jj, ss = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(ns), indexing="ij"))
    keys = fr.sample_keys(seed, jj * nx + ii, ss)
    u = (ii.astype(np.float32).astype(np.float64) + fr.draws(keys, 0, "f64")) / np.float64(nx)
    v = (jj.astype(np.float32).astype(np.float64) + fr.draws(keys, 1, "f64")) / np.float64(ny)
    rays = np.ascontiguousarray(probe_camera(np.stack([u, v], 1), keys)[:, :7])
    ctr = np.full(len(keys), 2, np.int64)
    if int(f.cam_kind) != 0:
        aperture, t0, t1 = (float(x) for x in f.cam[21:24])
        assert aperture == 0.0 and np.all(f.cam[:3] != 0.0), "a lens of real width moves the ray by what it drew"
        todo = np.ones(len(keys), bool)
        while todo.any():  # camera.clj / util.clj rand-in-unit-disk: retry while p . p >= 1
            x = 2.0 * fr.draws(keys[todo], ctr[todo], "f64") - 1.0
            y = 2.0 * fr.draws(keys[todo], ctr[todo] + 1, "f64") - 1.0
            ctr[todo] += 2
            todo[todo] = (x * x + y * y) + 0.0 >= 1.0
        rays[:, 6] = t0 + (t1 - t0) * fr.draws(keys, ctr, "f64")
        ctr += 1
    return rays, keys, ctr


def probe_frame_paths(probe_paths, rays, keys, ctr, depth, max_seg=0):
    """probe_paths(rays, keys, depth=, ctr0=, max_seg=) for paths that start at different draws: one call per distinct ctr -> (rgb, nseg, log, nlog)"""
    n = len(keys)
    rgb, nseg, nlog = np.zeros((n, 3)), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    log = np.zeros((n, max_seg, 12)) if max_seg else None
    for c in np.unique(ctr):
        pick = np.flatnonzero(ctr == c)
        out = probe_paths(rays[pick], keys[pick], depth=depth, ctr0=int(c), max_seg=max_seg)
        rgb[pick], nseg[pick], nlog[pick] = out[0], out[1], out[3]
        if max_seg:
            log[pick] = out[2]
    return rgb, nseg, log, nlog


def frame_of(rgb, nx, ny, ns):
    """the frame of these samples ([i, j, s] order): the in-order fold of core.clj:52-53 times 1 / ns -> [row, column, c], row 0 = top"""
    import frame_reference as fr
    return fr.frame_in_order(rgb.reshape(nx, ny, ns, 3))


def pixel_image(per_sample, nx, ny, ns):
    """a per-sample quantity in [i, j, s] order -> [row, column, s], row 0 = top (the layout of a frame)"""
    return np.ascontiguousarray(np.transpose(per_sample.reshape(nx, ny, ns), (1, 0, 2))[::-1])


# ---- the rules, as the depth-50 tests of these scenes state them, with the depth written in ---------------------------------------------------
MEDIA_SAME = 0.999   # test_media_match_oracle: share of the paths with the expected segment count
MEDIA_TOL = 1e-9     # ... and their logs and colours within this (a free-flight distance goes through log: ocml vs glibc, <= 1 ulp)


def check_paths(got, exp, exact, what):
    """probe_paths output against an expectation.  exact: bit equality of everything.  Otherwise test_media_match_oracle's rule for paths: at least
    99.9 % of the paths have the expected segment count; those have the expected primitives, logs within 1e-9 and colours within 1e-9."""
    rgb, nseg, log, nlog = got
    ergb, enseg, elog, enlog = exp
    if exact:
        assert np.array_equal(nseg, enseg), (what, "segments: %d of %d paths differ" % ((nseg != enseg).sum(), len(nseg)))
        assert np.array_equal(nlog, enlog), (what, "logged records")
        assert np.array_equal(log, elog), (what, "segment logs: %d paths differ" % (log != elog).any(axis=(1, 2)).sum())
        assert np.array_equal(rgb, ergb), (what, "colours: %d paths differ" % (rgb != ergb).any(axis=1).sum())
        return
    same = nseg == enseg
    assert same.mean() > MEDIA_SAME, (what, "%d of %d paths took another way" % ((~same).sum(), len(same)))
    assert np.array_equal(nlog[same], enlog[same]), (what, "logged records")
    assert np.array_equal(log[same][:, :, 0], elog[same][:, :, 0]), (what, "primitives of the logged segments")
    assert np.allclose(log[same], elog[same], rtol=MEDIA_TOL, atol=MEDIA_TOL), (what, "segment logs")
    assert np.allclose(rgb[same], ergb[same], atol=MEDIA_TOL, rtol=0), (what, "colours")


def check_frame_f64(got, exp, what):
    """test_render_matches_oracle / test_f3_scenes_match_nested_oracle: counters equal, rms < 1e-12, rgb8 within 1"""
    lin, q, cnt = got
    elin, eq, ecnt = exp
    assert np.array_equal(np.asarray(cnt, np.uint64), ecnt), (what, "total-rays / total-pixels", list(cnt), list(ecnt))
    assert rms(lin, elin) < 1e-12, (what, "rms", rms(lin, elin))
    assert np.abs(q.astype(int) - eq.astype(int)).max() <= 1, (what, "rgb8")


def check_frame_media(got, exp, d, what):
    """test_media_match_oracle's rule for frames with its one-path slack written for depth d: a free-flight distance within an ulp of the chord sends ONE
    path another way -- at most d + 1 segments of it against at least 1.  Two segments of slack, or d + 2 if at most one pixel moved; rms <= 1e-4."""
    lin, q, cnt = got
    elin, eq, ecnt = exp
    seg_diff = abs(int(cnt[0]) - int(ecnt[0]))
    moved = int((np.abs(lin - elin).max(axis=2) > MEDIA_TOL).sum())
    assert int(cnt[1]) == int(ecnt[1]), (what, "total-pixels")
    assert seg_diff <= 2 or (seg_diff <= d + 2 and moved <= 1), (what, "total-rays %d vs %d, %d pixels moved" % (int(cnt[0]), int(ecnt[0]), moved))
    assert rms(lin, elin) <= 1e-4, (what, "rms", rms(lin, elin))


def check_frame_f32(got, exp, d, what):
    """test_f32_random_scenes_match_f32_oracle's rule for frames with two paths' worth of segments written for depth d: sinf / powf (ocml vs glibc) can
    flip a checker sign or a Schlick draw -- at most 2 pixels differ by more than 1e-5, total-rays within 2 (d + 1)"""
    lin, q, cnt = got
    elin, eq, ecnt = exp
    moved = int((np.abs(lin - elin).max(axis=2) > 1e-5).sum())
    seg_diff = abs(int(cnt[0]) - int(ecnt[0]))
    assert moved <= 2, (what, "%d pixels differ from the f32 oracle's by more than 1e-5" % moved)
    assert seg_diff <= 2 * (d + 1), (what, "total-rays %d vs %d" % (int(cnt[0]), int(ecnt[0])))
    assert int(cnt[1]) == int(ecnt[1]), (what, "total-pixels")


def frames_equal(a, b):
    """two (linear, rgb8, counters) frames, bit for bit"""
    return all(np.array_equal(x, y) for x, y in zip(a, b))
