"""Shared by test_vol_host.py (CPU) and test_gpu_vol.py (GPU): the recipes of the volume rule's tests -- the three media scenes, their view rays, the
smoke box without its smoke, and the groups of the same-estimand tests, chosen by geometry alone.  Nothing here imports the device library; the oracle
is passed in.  Not a test module (pytest collects test_*.py only).

Media scenes by name:
  "smoke"       nee_cases.media_flat(): the Cornell box whose blocks are smoke, white (albedo 1) and black (albedo 0), under a 330 x 305 rectangle lamp;
  "subsurface"  scene.make_subsurface_sphere: a glass ball filled with a blue medium inside a sphere lamp of radius 1000 seen from inside;
  "final"       depth_cases' "final": make-final, one ceiling lamp seen through a haze that fills the world, a moving sphere, a medium in a glass ball."""
import functools

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import hitable as hit
from raytrace_clj_amd import util
from tests import depth_cases as dc
from tests import direct_cases as dcs
from tests import nee_cases as ncs

MEDIA_SCENES = ("smoke", "subsurface", "final")
DEPTHS = ncs.DEPTHS
ESTIMATORS = ((1, 0), (2, 0), (2, 1))  # (estimator, light_choice): the NEE rule does not look at the choice
SHAPES = ((13, 7, 3), (40, 24, 2))     # 273 rows: nx no multiple of 8, a partial last wave; 30 full waves
ESTIMAND_G, ESTIMAND_N, ESTIMAND_DEPTH, ESTIMAND_SEED = ncs.ESTIMAND_G, ncs.ESTIMAND_N, 3, 0x564F4C


@functools.lru_cache(maxsize=None)
def flat(name):
    from oracle.tree import flatten_with_tree
    if name == "smoke":
        return ncs.media_flat()
    if name == "subsurface":
        return flatten_with_tree(r.scene.make_subsurface_sphere(dcs.NX, dcs.NY))
    assert name == "final", name
    return dc.flat("final")


@functools.lru_cache(maxsize=None)
def view_rays(oracle, name, n=dcs.N_POINTS):
    """n camera rays of the scene through uniform random film points; do not write into them"""
    rng = np.random.default_rng(37)
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    return np.ascontiguousarray(oracle.probe_camera(flat(name), rng.random((n, 2)), keys)[:, :7])


# ---- the smoke box, piece by piece (scene.make_cornell_box(classic=False)'s numbers) ----------------------------------------------------------------
LAMP = (113.0, 127.0, 443.0, 432.0, 554.0)                            # rect_xz x0, z0, x1, z1, k
BLOCKS = (((165.0, 165.0, 165.0), -18.0, (130.0, 0.0, 65.0)),         # the white smoke: box size, rotate-y angle, offset
          ((165.0, 330.0, 165.0), 15.0, (265.0, 0.0, 295.0)))         # the black smoke


@functools.lru_cache(maxsize=None)
def clear_flat():
    """the smoke box with both media removed: its walls and its lamp alone (what a shadow ray that ignores the media sees)"""
    from oracle.tree import flatten_with_tree
    sc = r.scene.make_cornell_box(dcs.NX, dcs.NY, classic=False)
    items = [it for it in _items(sc["world"]) if not isinstance(it, hit.ConstantMedium)]
    assert len(items) == 6
    return flatten_with_tree({"camera": sc["camera"], "world": hit.make_bvh(items, 0.0, 1.0, util.SplitMix64(1))})


def _items(node):
    """the leaves of a make_bvh tree, left to right"""
    if isinstance(node, hit.bvh_node):
        return _items(node.left) + ([] if node.right is node.left else _items(node.right))
    return [node]


def block_chord(k, origin, direction):
    """the chord of rays origin + t * direction (t >= 0, [n, 3] each) through smoke block k -> (t_in, t_out), t_in >= t_out where the ray misses: the
    slab test in the block's own frame (the reference rotates about y by theta, then translates)"""
    size, theta, offset = BLOCKS[k]
    c, s = np.cos(np.radians(theta)), np.sin(np.radians(theta))

    def local(v):  # the inverse of rotate-y(theta): x' = c x - s z, z' = s x + c z
        return np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], axis=1)
    o, d = local(np.asarray(origin, np.float64) - np.asarray(offset)), local(np.asarray(direction, np.float64))
    with np.errstate(all="ignore"):
        a, b = (0.0 - o) / d, (np.asarray(size) - o) / d
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return np.maximum(np.nanmax(lo, axis=1), 0.0), np.nanmin(hi, axis=1)


def media_lie_below_the_lamp():
    """every medium of the smoke box lies wholly on the near side of the lamp's plane: the far end of a shadow ray's interval never cuts a chord"""
    return all(off[1] + size[1] < LAMP[4] for size, _, off in BLOCKS)


@functools.lru_cache(maxsize=None)
def estimand_inputs(oracle, groups=ESTIMAND_G, n=ESTIMAND_N):
    """-> (rays [groups * n, 7], keys [groups * n], kind [groups]: 0 = smoke, 1 = floor).  Half the groups are view rays whose chord through the WHITE
    smoke is at least 150 units and that enter it before anything else: 78 % or more of their paths scatter there first (1 - exp(-0.01 * 150)), so
    their first vertex is an Isotropic scatter in the white smoke, and the shadow ray from it starts inside the block.  The other half are view rays
    that miss both blocks and reach the floor (y = 0) at a point whose segment to the lamp's centre crosses a block over at least 50 units.  The choice
    reads the geometry alone, no radiance.  Path r of group g is keyed sample_key(ESTIMAND_SEED, g, r)."""
    view = view_rays(oracle, "smoke", 6000)
    o, d = view[:, 0:3], view[:, 3:6]
    norm = np.sqrt((d * d).sum(axis=1))
    t0, t1 = block_chord(0, o, d)
    b0, b1 = block_chord(1, o, d)
    misses_black = ~(b1 > b0) | (b0 > t0)
    smoke = (t1 > t0) & ((t1 - t0) * norm >= 150.0) & misses_black
    rec = oracle.probe_hit(clear_flat(), view, tmin=0.001)
    p = rec[:, 3:6]
    floor = (rec[:, 0] != 0.0) & (np.abs(p[:, 1]) < 1e-9) & ~(t1 > t0) & ~(b1 > b0)
    centre = np.array([(LAMP[0] + LAMP[2]) / 2, LAMP[4], (LAMP[1] + LAMP[3]) / 2])
    to = centre[None, :] - p
    length = np.sqrt((to * to).sum(axis=1))
    crossed = np.zeros(len(view))
    for k in range(2):
        c0, c1 = block_chord(k, p, to)
        crossed = np.maximum(crossed, np.where(c1 > c0, (np.minimum(c1, 1.0) - c0) * length, 0.0))
    floor &= crossed >= 50.0
    half = groups // 2
    chosen = np.concatenate([np.flatnonzero(smoke)[:half], np.flatnonzero(floor)[:groups - half]])
    assert len(chosen) == groups, (int(smoke.sum()), int(floor.sum()))
    kind = np.concatenate([np.zeros(half, np.int64), np.ones(groups - half, np.int64)])
    rays = np.ascontiguousarray(np.repeat(view[chosen], n, axis=0))
    g, k = (a.ravel() for a in np.meshgrid(np.arange(groups), np.arange(n), indexing="ij"))
    return rays, util.sample_keys(ESTIMAND_SEED, g, k), kind
