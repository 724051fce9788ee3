"""Shared by test_nee_host.py (CPU) and test_gpu_nee.py (GPU): the recipes the light-sampled path tests add to tests/direct_cases.py (imported, not
edited).  Nothing here imports the device library; the oracle is passed in.  Not a test module (pytest collects test_*.py only)."""
import functools

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd import util
from tests import direct_cases as dcs

CASES = (("example-light", "f64"), ("cornell", "f64"), ("sphere-lamp", "f64"), ("sphere-lamp", "f32"))
DEPTHS = (0, 1, 3, 50)
ESTIMAND_SCENE, ESTIMAND_DEPTH, ESTIMAND_SEED = "sphere-lamp", 3, 0x4E45
ESTIMAND_G, ESTIMAND_N = 48, 4096  # groups and paths per group of the same-estimand tests (see test_nee_host.test_same_estimand's docstring)


@functools.lru_cache(maxsize=None)
def path_keys(n=dcs.N_POINTS):
    """one stream key per view ray; do not write into them"""
    return np.random.default_rng(31).integers(0, 2 ** 63, n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def media_flat():
    """the Cornell box whose blocks are smoke: a scene the light-sampled paths refuse"""
    from oracle.tree import flatten_with_tree
    return flatten_with_tree(r.scene.make_cornell_box(dcs.NX, dcs.NY, classic=False))


@functools.lru_cache(maxsize=None)
def estimand_inputs(oracle, groups=ESTIMAND_G, n=ESTIMAND_N):
    """-> (rays [groups * n, 7], keys [groups * n]): the first `groups` view rays of the estimand scene whose first hit is Lambertian and sees the lamp
    under a fair share of its scatter lobe, each repeated n times; path r of group g is keyed sample_key(ESTIMAND_SEED, g, r), what the render calls
    derive without keys.  The share: z_g takes both group means for normal, and the plain estimator's is only once a good number of its n paths have
    found the lamp.  A bounce finds a sphere lamp (centre c, radius rad) with probability about 2 cos^3 / pi x pi rad^2 / |c - p|^2 -- the lobe at the
    lamp's centre times its projected disk -- so a first hit qualifies when that is >= 0.02 (some 80 of 4096 paths); a point 15 units away, where it is
    7e-4, would see the lamp from three paths and often from none, and its z_g would divide by a variance of zero.  The choice reads the geometry
    alone, no radiance."""
    f = dcs.flat(ESTIMAND_SCENE)
    view = dcs.view_rays(oracle, ESTIMAND_SCENE)
    rec = dcs.oracle_records(oracle, ESTIMAND_SCENE, view)
    lamb = (rec[:, 0] != 0.0) & (np.asarray(f.mat_kind, np.int64)[rec[:, 11].astype(np.int64)] == fl.MAT_LAMBERTIAN)
    lamp = np.asarray(f.prim_geom, np.float64).reshape(-1, 9)[len(f.prim_kind) - 1]
    to = lamp[0:3] - rec[:, 3:6]
    d2 = (to * to).sum(axis=1)
    with np.errstate(all="ignore"):
        cos = (rec[:, 6:9] * to).sum(axis=1) / np.sqrt(d2 * (rec[:, 6:9] ** 2).sum(axis=1))
        lamb &= (cos > 0.0) & (2.0 * cos ** 3 * lamp[3] ** 2 / d2 >= 0.02)
    chosen = np.flatnonzero(lamb)[:groups]
    assert len(chosen) == groups
    rays = np.ascontiguousarray(np.repeat(view[chosen], n, axis=0))
    g, k = (a.ravel() for a in np.meshgrid(np.arange(groups), np.arange(n), indexing="ij"))
    return rays, util.sample_keys(ESTIMAND_SEED, g, k)
