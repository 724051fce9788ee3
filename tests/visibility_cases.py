"""Shared by test_visibility_host.py (CPU) and test_gpu_visibility.py (GPU): the scenes and ray sets of the closest-hit / any-hit query tests.
Nothing here imports the device library; the oracle is passed in.  Not a test module (pytest collects test_*.py only).

Scenes by name: the worlds of tests/depth_cases.py ("cover" -- a thin lens, MovingSpheres, shutter [0, 1] --, "cornell", "final", "hitlist-media")
and the recipes of tests/tree_scenes.py.  Ray sets, N rays each (47 waves, the last one partial):
  camera rays (depth_cases.camera_paths) for the depth_cases worlds, tree_scenes.cloud_rays / chain_rays for the recipes, and in the second half of
  every set "second-segment" rays: from the oracle's hit points of the first half, along camera.hemisphere_rays directions about the hit normal --
  what an ambient-occlusion or shadow pass sends."""
import functools

import numpy as np

from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import flatten as fl
from tests import depth_cases as dc
from tests import tree_scenes as ts

N = 3000
FLT_MAX = 3.4028234663852886e38
SEED = 0x5EED0002
DEPTH_SCENES = ("cover", "cornell", "final", "hitlist-media")
TREE_SCENES = ("layer(256)", "cloud(129)", "chain(1000, 0.9, 0.15)", "many_big(20, 300)", "mixed(65)")
SCENES = DEPTH_SCENES + TREE_SCENES
SPHERE_SCENES = ("cover", "layer(256)", "cloud(129)", "chain(1000, 0.9, 0.15)", "many_big(20, 300)")  # worlds RTMI_F32 traces
MEDIA_SCENES = ("final", "hitlist-media")  # a free-flight distance goes through log (ocml vs glibc): the device is compared with itself there
CHAIN = (1000, 0.9, 0.15)
# the ranges of the flag tests: the default, an ambient-occlusion radius, the behind-the-origin path (t-min < 0), an empty interval
RANGES = ((0.001, FLT_MAX), (0.001, 1.0), (-1.0, 5.0), (0.5, 0.5))


@functools.lru_cache(maxsize=None)
def flat(name):
    """the scene flattened (with its nested world for the oracle where the world is more than spheres)"""
    if name in DEPTH_SCENES:
        return dc.flat(name)
    if name.startswith("mixed"):
        from oracle.tree import flatten_with_tree
        return flatten_with_tree(ts.scene(ts.mixed(int(name[6:-1]))))
    if name.startswith("chain"):
        return fl.flatten(ts.chain_scene(ts.build(name)))
    return fl.flatten(ts.scene(ts.build(name)))


def second_segment_rays(oracle, f, rays, n_dirs=1, seed=SEED, tmin=0.001, tmax=FLT_MAX):
    """n_dirs rays from every hit point of `rays` (the oracle's closest hits), cosine-weighted about the normal turned towards the ray's origin;
    time = the first ray's.  -> rays [hits * n_dirs, 7]"""
    h = oracle.probe_hit(f, rays, tmin=tmin, tmax=tmax)
    hit = h[:, 0] == 1
    p, n = h[hit, 3:6], h[hit, 6:9].copy()
    away = (n * rays[hit, 3:6]).sum(axis=1) > 0.0
    n[away] = -n[away]
    ok = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & ((n * n).sum(axis=1) > 0.0)
    out = cam.hemisphere_rays(p[ok], n[ok], n_dirs, seed=seed)
    out[:, 6] = np.repeat(rays[hit, 6][ok], n_dirs)
    return out


def _first_half(oracle, name):
    if name in DEPTH_SCENES:
        rays = dc.camera_paths(oracle, name, n=N)[0].copy()
        if name == "cover":  # the trees were built for the shutter [0, 1]: a third of the rays outside it (the exact MovingSphere pass)
            rays[0::3, 6] = 1.5 + rays[0::3, 6]
        return rays
    if name.startswith("chain"):
        return ts.chain_rays(*CHAIN, N - 300, 41, n_fallback=300)[0]  # (the last 300: not boundable in float -- the exact flat-scan fallback)
    return ts.cloud_rays(N, 67)


_rays = {}


def rays(oracle, name):
    """the scene's N rays: the first half primary rays, the second half second-segment rays of their hits (as many as there are; the rest primary)"""
    if name not in _rays:
        first = _first_half(oracle, name)
        sec = second_segment_rays(oracle, flat(name), first[:N // 2])[:N // 2]
        _rays[name] = np.ascontiguousarray(np.concatenate([first[:N - len(sec)], sec]))
        assert _rays[name].shape == (N, 7)
    return _rays[name]


def keys(n=N, seed=5):
    return np.random.default_rng(seed).integers(0, 2 ** 63, n, dtype=np.uint64)


# ---- the ray set of "the exit is real": second-segment rays INSIDE a layer of spheres with no dome around it, unbounded range ------------------
COUNT_SCENE = "layer(256, dome=False)"


@functools.lru_cache(maxsize=None)
def count_flat():
    return fl.flatten(ts.scene(ts.layer(256, dome=False)))


_count_rays = {}


def count_rays(oracle):
    """N rays that start on the layer's spheres (the hit points of rays shot through the layer from its side) and leave about the surface normal,
    of which those are kept that start well inside the layer and are still between the spheres' feet and heads six units on: a ray that stays low
    crosses many cells of the entry grid with spheres in them -- the closest-hit search must settle which is nearest, the any-hit search may leave
    at the first."""
    if "r" not in _count_rays:
        rng = np.random.default_rng(71)
        m = 8 * N
        o = np.stack([np.full(m, -12.0), rng.uniform(0.05, 0.35, m), rng.uniform(-9.0, 9.0, m)], axis=1)
        d = np.stack([np.ones(m), rng.normal(0, 0.01, m), rng.normal(0, 0.3, m)], axis=1)
        side = np.concatenate([o, d, np.zeros((m, 1))], axis=1)
        sec = second_segment_rays(oracle, count_flat(), side, n_dirs=32, seed=SEED + 1)
        end = sec[:, 1] + 6.0 * sec[:, 4]
        low = (end > 0.02) & (end < 0.38) & (np.abs(sec[:, 0]) < 7.0) & (np.abs(sec[:, 2]) < 7.0)
        _count_rays["r"] = np.ascontiguousarray(sec[low][:N])
        assert _count_rays["r"].shape == (N, 7), _count_rays["r"].shape
    return _count_rays["r"]
