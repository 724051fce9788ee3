"""The ray depth limit on the CPU: the oracle's handling of `depth` against the prefix rule (depth_cases.py: core.clj:25-41 restated over the oracle's own
depth-50 paths, without its depth argument), and the conditions under which the frames test_gpu_depth.py renders can tell a limit from its neighbours.

Why.  At depth 50 -- the limit of every other frame of the suite -- the per-lane depth counter of the trace kernels decides almost nothing: of 20 000
camera paths of the cover scene one reaches the limit, and the frames at depth 49 and 50 are equal pixel for pixel and in total-rays.  At depths 0 .. 3
it decides most samples.  The conditions below are floors, not measurements: a frame pair that fell under them could hide an off-by-one inside a tolerance.

Measured here (8192 paths per scene; share of the paths whose last segment is the one traced with the counter at 0 / share the limit actually cuts; then
total-rays and rms between the oracle's frames at d and d + 1):
  cover 64x32x8     d=0 100 % / 83 %  13530, 0.317   d=1 83 % / 32 %  5231, 0.113   d=2 32 % / 16 %  2589, 0.0702   d=3 16 % / 7.7 %  1203, 0.0163
  cover 61x37x7     d=0               13048, 0.324   d=1              4902, 0.112   d=2              2445, 0.0755   d=3               1133, 0.0157
  cornell 48x48x8   d=0 100 % / 91 %  16641, 0.121   d=1 91 % / 62 %  11482, 0.0671 d=2 62 % / 51 %  9510, 0.0375  d=3 51 % / 42 %  7883, 0.0235
  final 48x48x4     d=0 100 % / 70 %  6370, 0.275    d=1 70 % / 44 %  4051, 0.139   d=2 44 % / 29 %  2616, 0.130   d=3 29 % / 20 %  1752, 0.0587
  hitlist-media     d=0 100 % / 68 %  11133, 0.339   d=1 68 % / 20 %  3377, 0.0855  d=2 20 % / 13 %  2275, 0.0594  d=3 13 % / 8.0 %  1391, 0.0341
  narrowed-media    d=0 100 % / 93 %  15280, 0.168   d=1 93 % / 73 %  12007, 0.138  d=2 73 % / 57 %  9157, 0.106   d=3 57 % / 42 %  6810, 0.0831"""
import numpy as np
import pytest

import depth_cases as dc

LIMIT_SHARE = 0.10   # at least this share of a scene's paths ends at the limit ...
RAYS_APART = 1000    # ... and the frames at neighbouring limits differ by at least this many segments ...
RMS_APART = 1e-3     # ... and by this rms: nine orders above the FP64 frame tolerance (1e-12), one above the media one (1e-4)


def _paths50(oracle, name):
    rays, keys, ctr0 = dc.camera_paths(oracle, name)
    return oracle.probe_paths(dc.flat(name), rays, keys, depth=dc.FULL, ctr0=ctr0, max_seg=dc.LOG50)


def test_prefix_expectation_on_paths_written_by_hand():
    """the rule itself: a path that misses at once, one that ends on a light at its second segment, one that misses at its third, one cut at 51"""
    rec = lambda prim, scat: [prim, 1.5, 1, 2, 3, 0, 1, 0] + ([0.5, 0.5, 0.5, 1] if scat else [0, 0, 0, 0])
    zero = [0.0] * 12
    log50 = np.array([[zero, zero, zero, zero], [rec(3, True), rec(0, False), zero, zero], [rec(3, True), rec(4, True), zero, zero],
                      [rec(5, True), rec(6, True), rec(7, True), rec(8, True)]])
    rgb50 = np.array([[0, 0, 0], [0.5, 0.7, 1.0], [0, 0, 0], [0, 0, 0.0]])
    nseg50 = np.array([1, 2, 3, 51], np.uint64)
    rgb, nseg, log, nlog = dc.prefix_expectation(rgb50, nseg50, log50, 0)
    assert list(nseg) == [1, 1, 1, 1] and list(nlog) == [0, 1, 1, 1] and not rgb.any() and log.shape == (4, 1, 12)
    assert list(log[1, 0]) == rec(3, False) and list(log[3, 0]) == rec(5, False)          # cut: hit kept, no scattered direction
    rgb, nseg, log, nlog = dc.prefix_expectation(rgb50, nseg50, log50, 1)
    assert list(nseg) == [1, 2, 2, 2] and list(nlog) == [0, 2, 2, 2] and list(rgb[1]) == [0.5, 0.7, 1.0] and not rgb[[0, 2, 3]].any()
    assert list(log[1, 1]) == rec(0, False) and list(log[2, 0]) == rec(3, True) and list(log[2, 1]) == rec(4, False)
    rgb, nseg, log, nlog = dc.prefix_expectation(rgb50, nseg50, log50, 2)
    assert list(nseg) == [1, 2, 3, 3] and list(nlog) == [0, 2, 2, 3] and list(log[2, 1]) == rec(4, True) and list(log[3, 2]) == rec(7, False)
    rgb, nseg, log, nlog = dc.prefix_expectation(rgb50, nseg50, log50, 3)
    assert list(nseg) == [1, 2, 3, 4] and list(log[3, 2]) == rec(7, True) and list(log[3, 3]) == rec(8, False)


@pytest.mark.parametrize("name", list(dc.SCENES))
def test_oracle_depth_is_the_prefix_of_its_depth_50_paths(oracle, name):
    """oracle.probe_paths at every depth of depth_cases against prefix_expectation of its own depth-50 run: bit for bit on the sphere and rectangle worlds, by
    test_media_match_oracle's rule for paths on the worlds that hold media"""
    f, exact = dc.flat(name), dc.SCENES[name][3]
    rays, keys, ctr0 = dc.camera_paths(oracle, name)
    rgb50, nseg50, log50, _ = _paths50(oracle, name)
    assert nseg50.max() == dc.FULL + 1 or name == "cover"   # (every scene but the cover scene has paths that run into depth 50 itself)
    for d in dc.DEPTHS:
        got = oracle.probe_paths(f, rays, keys, depth=d, ctr0=ctr0, max_seg=dc.max_seg(d))
        dc.check_paths(got, dc.prefix_expectation(rgb50, nseg50, log50, d), exact, (name, "depth", d))
        assert got[1].max() == d + 1


@pytest.mark.parametrize("name", list(dc.SCENES))
def test_gpu_depth_inputs_discriminate(oracle, name):
    """For every scene, shape and depth <= 3 of test_gpu_depth.py: at least 10 % of the scene's 8192 paths end at the limit, and the oracle's frames at d and
    d + 1 (and so at d and d - 1) differ by at least 1000 in total-rays and 1e-3 in rms"""
    _, nseg50, _, _ = _paths50(oracle, name)
    for d in range(4):
        share, cut = dc.limit_share(nseg50, d), dc.cut_share(nseg50, d)
        print("%s depth %d: %.1f %% of the paths end at the limit, %.1f %% are cut by it" % (name, d, 100 * share, 100 * cut))
        assert share >= LIMIT_SHARE, (name, d, share)
    for shape in dc.SCENES[name][1]:
        for d in range(4):
            a, b = dc.oracle_frame(oracle, name, shape, d), dc.oracle_frame(oracle, name, shape, d + 1)
            rays, apart = int(b[2][0]) - int(a[2][0]), dc.rms(a[0], b[0])
            print("%s %dx%dx%d depth %d vs %d: total-rays %+d, rms %.4g" % ((name,) + shape + (d, d + 1, rays, apart)))
            assert rays >= RAYS_APART and apart >= RMS_APART, (name, shape, d, rays, apart)
        assert int(dc.oracle_frame(oracle, name, shape, 0)[2][0]) == shape[0] * shape[1] * shape[2]   # depth 0: one segment per sample


def test_depth_1000_is_the_unlimited_cover_frame(oracle):
    """No path of the cover frame has 1000 segments, so depth 1000 renders the unlimited frame; it differs from the depth-50 frame in the pixels of the
    paths that ran into depth 50 and nowhere else.  The frame's samples are taken one by one from the probes (depth_cases.frame_paths) -- and must
    fold to the frames oracle.render returns, bit for bit."""
    name, (nx, ny, ns) = "cover", dc.SCENES["cover"][1][0]
    f = dc.flat(name)
    rays, keys, ctr = dc.frame_paths(lambda uv, k: oracle.probe_camera(f, uv, k), f, nx, ny, ns)
    probe = lambda *a, **kw: oracle.probe_paths(f, *a, **kw)
    rgb50, nseg50, _, _ = dc.probe_frame_paths(probe, rays, keys, ctr, dc.FULL)
    rgb1k, nseg1k, _, _ = dc.probe_frame_paths(probe, rays, keys, ctr, dc.DEEP)
    f50, f1k = dc.oracle_frame(oracle, name, (nx, ny, ns), dc.FULL), dc.oracle_frame(oracle, name, (nx, ny, ns), dc.DEEP)
    assert np.array_equal(dc.frame_of(rgb50, nx, ny, ns), f50[0]) and int(nseg50.sum()) == int(f50[2][0])
    assert np.array_equal(dc.frame_of(rgb1k, nx, ny, ns), f1k[0]) and int(nseg1k.sum()) == int(f1k[2][0])
    assert nseg1k.max() < dc.DEEP, "a path of %d segments: depth 1000 is a limit after all" % nseg1k.max()
    reached = dc.pixel_image(nseg1k > dc.FULL + 1, nx, ny, ns).any(axis=2)   # pixels with a sample the limit of 50 cut
    print("cover %dx%dx%d: longest path %d segments, %d paths ran into depth 50" % (nx, ny, ns, nseg1k.max(), int((nseg1k > dc.FULL + 1).sum())))
    assert np.array_equal(f1k[0][~reached], f50[0][~reached]) and np.array_equal(f1k[1][~reached], f50[1][~reached])
    assert np.array_equal(nseg1k <= dc.FULL + 1, nseg1k == nseg50) and np.array_equal(np.minimum(nseg1k, dc.FULL + 1), nseg50)
