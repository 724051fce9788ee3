"""Shared by test_mis_host.py (CPU) and test_gpu_mis.py (GPU): the recipes the MIS tests add to tests/nee_cases.py and tests/direct_cases.py (imported,
not edited).  Nothing here imports the device library; the oracle is passed in.  Not a test module (pytest collects test_*.py only).

THE NEAR SET.  near_inputs picks, by geometry alone (no radiance is read), Lambertian first hits on the sphere-lamp scene's floor: camera rays through
40 000 random film points, those that land on the floor, in film order, whose share of the scatter lobe taken by the lamp -- 2 cos^3 rad^2 / |c - p|^2,
nee_cases.estimand_inputs' measure -- is at least NEAR_SHARE; the first G = 48 of them, n = 4096 paths each, depth 3 (the far set's counts).
NEAR_SHARE was found on the CPU (oracle paths, the rule restated by tests/mis_reference.py) by raising the share in steps of 0.01 from 0 until the
correct rule passes the z-test (|mean z| <= 4 / sqrt(G) = 0.577, max |z| <= 5) while control A (the weighted closing emissions are dropped) and control
B (they are kept whole) both fail it.  Recorded before any device ran, light choice 0 (the scene has one light, so choice 1 picks the same light
with the same q = 1 and gave the same figures to the last digit):
  share >= 0.00: the correct rule FAILS (mean z 6.746, max |z| 42.58): groups whose plain paths never find the lamp have no variance to divide by;
  share >= 0.01: correct mean z 0.034, max |z| 3.19; control A mean z -3.610 (max 11.40); control B mean z 8.383 (max 11.38)   <- NEAR_SHARE
  every step from 0.02 to 0.16: correct |mean z| <= 0.164, max |z| <= 2.50; A mean z from -3.60 down to -8.94; B mean z from 8.47 up to 10.03.
The issue expected control A to pass on the far set (nee_cases.estimand_inputs, share >= 0.02); it does not (correct 0.002 / 1.86, A -3.717 / 17.97,
B 8.375 / 11.44), which is why the smallest share that separates the rules is so low.  A set that low is not near the lamp in any plain sense, so the
tests also run UNDER_SHARE = 0.16, the floor right under the lamp, where the density ratio x is of order one (8 cos^3 cos' rad^2 / d^2 = 1.5 straight
below it) and the closing weight carries as much as the light sample: correct 0.044 / 1.55, A -8.937 / 11.93, B 10.030 / 11.67."""
import functools

import numpy as np

from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd import util
from tests import direct_cases as dcs
from tests import nee_cases as ncs

CASES, DEPTHS = ncs.CASES, ncs.DEPTHS
CHOICES = (0, 1)
NEAR_G, NEAR_N = ncs.ESTIMAND_G, ncs.ESTIMAND_N
NEAR_SEED = 0x4D4953
NEAR_SHARE, UNDER_SHARE = 0.01, 0.16

# the planar check of the issue: the shaded point at the origin, normal +z, an unoccluded rect_xy light of unit emission in the plane z = h
PLANAR = ((1.0, (1.0, -52.0, 131.0, 53.0)),    # the Cornell lamp, one unit away from its edge
          (3.0, (-1.0, -1.0, 1.0, 1.0)),
          (0.2, (0.1, -1.0, 2.0, 1.0)))
PLANAR_N = 1 << 20


def planar_table(h, rect):
    x0, y0, x1, y1 = rect
    return np.array([[3.0, x0, y0, x1, y1, h, abs((x1 - x0) * (y1 - y0)), 1.0, 1.0, 1.0]])


def unit_ball(rng, n):
    """n points uniform in the unit ball (a direction times the cube root of a uniform: no rejection, any count)"""
    v = rng.normal(size=(n, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    return v * np.cbrt(rng.random(n))[:, None]


def planar_scatter(h, rect, n, seed):
    """n scatters n + b from the origin -> (hit [n] bool: the ray meets the rectangle, D [n, 3], t [n])"""
    D = unit_ball(np.random.default_rng(seed), n) + np.array([0.0, 0.0, 1.0])
    with np.errstate(all="ignore"):
        t = h / D[:, 2]
        x, y = t * D[:, 0], t * D[:, 1]
    hit = (D[:, 2] > 0.0) & (x >= rect[0]) & (x <= rect[2]) & (y >= rect[1]) & (y <= rect[3])
    return hit, D, t


def planar_terms(h, rect, n=PLANAR_N, seed=7):
    """-> dict of per-sample arrays [n]: plain (1 where an independent scatter finds the lamp), nee (w), light (m of the light sample), emission (m' of a
    scatter that finds the lamp, 0 where it misses), whole (1 where that scatter finds the lamp: control B's emission part)"""
    table = planar_table(h, rect)
    rng = np.random.default_rng(seed)
    ks, kp = rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    p, nrm = np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1))
    l, q, live = cam.mis_pick(table, kp, 0)
    _, d, w, built = cam.nee_samples(p, nrm, table, ks, kp, light=l)
    x, m = cam.mis_weight(w, q[l])
    plain = planar_scatter(h, rect, n, seed + 1)[0].astype(np.float64)
    hit, D, t = planar_scatter(h, rect, n, seed + 2)
    g = cam.mis_lobe(nrm, D)
    xq, mq = cam.mis_closing(g, nrm, D, t, table[0, 6], q[0])
    return dict(plain=plain, nee=w, light=m, emission=np.where(hit, mq, 0.0), whole=hit.astype(np.float64), x=x)


def lamp_share(f, rec):
    """the share of the scatter lobe the sphere lamp (the scene's last primitive) takes, seen from the records' points: 2 cos^3 rad^2 / |c - p|^2 -- the
    lobe at the lamp's centre times its projected disk (nee_cases.estimand_inputs' measure); 0 where the lamp is behind the point"""
    lamp = np.asarray(f.prim_geom, np.float64).reshape(-1, 9)[len(f.prim_kind) - 1]
    to = lamp[0:3] - rec[:, 3:6]
    d2 = (to * to).sum(axis=1)
    with np.errstate(all="ignore"):
        cos = (rec[:, 6:9] * to).sum(axis=1) / np.sqrt(d2 * (rec[:, 6:9] ** 2).sum(axis=1))
        return np.where(cos > 0.0, 2.0 * cos ** 3 * lamp[3] ** 2 / d2, 0.0)


@functools.lru_cache(maxsize=None)
def near_candidates(oracle, count=40000):
    """camera rays of the estimand scene through `count` uniform random film points (a seed of their own) whose first hit is the Lambertian floor
    -> (rays [m, 7], share [m]) in film order; do not write into them"""
    f = dcs.flat(ncs.ESTIMAND_SCENE)
    rng = np.random.default_rng(NEAR_SEED)
    keys = rng.integers(0, 2 ** 63, count, dtype=np.uint64)
    view = np.ascontiguousarray(oracle.probe_camera(f, rng.random((count, 2)), keys)[:, :7])
    rec = dcs.oracle_records(oracle, ncs.ESTIMAND_SCENE, view)
    ground = int(np.flatnonzero(np.asarray(f.prim_geom, np.float64).reshape(-1, 9)[:, 3] == 1000.0)[0])  # the sphere of radius 1000
    floor = (rec[:, 0] != 0.0) & (rec[:, 1] == float(ground)) & (np.asarray(f.mat_kind, np.int64)[rec[:, 11].astype(np.int64)] == fl.MAT_LAMBERTIAN)
    return view[floor], lamp_share(f, rec[floor])


@functools.lru_cache(maxsize=None)
def near_inputs(oracle, share=None, groups=NEAR_G, n=NEAR_N):
    """-> (rays [groups * n, 7], keys [groups * n]): the first `groups` floor candidates whose lamp share is >= share (NEAR_SHARE), each repeated n times;
    path r of group g is keyed sample_key(NEAR_SEED, g, r), what the render calls derive without keys"""
    view, s = near_candidates(oracle)
    chosen = np.flatnonzero(s >= (NEAR_SHARE if share is None else share))[:groups]
    assert len(chosen) == groups, len(chosen)
    rays = np.ascontiguousarray(np.repeat(view[chosen], n, axis=0))
    g, k = (a.ravel() for a in np.meshgrid(np.arange(groups), np.arange(n), indexing="ij"))
    return rays, util.sample_keys(NEAR_SEED, g, k)


def two_lamp_scene(second=(4.0, 4.0, 4.0)):
    """scene.make_example_light with a material of its own on the rectangle lamp, emitting `second`: the same primitives in the same tree, so one
    scene is a material edit of the other"""
    import raytrace_clj_amd as r
    from raytrace_clj_amd import hitable as hit
    from raytrace_clj_amd import shader as shad
    from raytrace_clj_amd import texture as tex
    from raytrace_clj_amd.scene import SCENE_SEED
    from raytrace_clj_amd.util import SplitMix64, vec3
    gray = shad.lambertian(albedo=tex.constant(color=vec3(0.6, 0.6, 0.6)))
    ball = shad.diffuse_light(tex=tex.constant(color=vec3(4, 4, 4)))
    panel = shad.diffuse_light(tex=tex.constant(color=vec3(*second)))
    return {"camera": r.camera.thin_lens_camera(lookfrom=vec3(13, 2, 3), lookat=vec3(0, 1, 0), vup=vec3(0, 1, 0), vfov=40, aspect=float(dcs.NX) / float(dcs.NY),
                                                aperture=0.0, focus_dist=10.0, t0=0.0, t1=1.0),
            "world": hit.make_bvh([hit.sphere(center=vec3(0, -1000, 0), radius=1000, material=gray), hit.sphere(center=vec3(0, 2, 0), radius=2, material=gray),
                                   hit.sphere(center=vec3(0, 7, 0), radius=2, material=ball), hit.rect_xy(x0=3, y0=1, x1=5, y1=3, k=-2, material=panel)],
                                  0.0, 1.0, SplitMix64(SCENE_SEED))}


def two_lamp_flat(second=(4.0, 4.0, 4.0)):
    from oracle.tree import flatten_with_tree
    return flatten_with_tree(two_lamp_scene(second))
