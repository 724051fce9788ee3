"""Shared by test_ris_host.py (CPU) and test_gpu_ris.py (GPU): the recipes of the proposal-rule tests, built with the Python mirror only, on top of
tests/direct_cases.py, nee_cases.py and mis_cases.py (imported, not edited).  Nothing here imports the device library; the oracle is passed in.  Not a
test module (pytest collects test_*.py only).

Scenes by name:
  "lamps8"         a ground sphere, a Lambertian, a metal and a glass ball under EIGHT lamps in three colours, one of them with zero emission: two Sphere,
                   one UVSphere, one each of rect_xy, rect_xz and rect_yz, and two small spheres close to the floor; flattened with a tree: mixed-kind FP64;
  "lamps-spheres"  the sphere-lamp scene's balls under five Sphere lamps, one switched off: sphere lamps only, what the sphere kernels and RTMI_F32 trace;
  "lamps32"        about 100 small spheres plus 32 sphere lamps, all listed; lamps32_flat(33) is the 33-lamp variant the error check wants.
The one-lamp cases are nee_cases.CASES, unchanged.

THE NEAR SET.  near_inputs picks, by geometry alone (no radiance is read), Lambertian first hits on lamps8's floor next to its two low lamps: camera rays
through 40 000 random film points, those that land on the ground sphere, in film order, whose share of the scatter lobe taken by the nearer of the two low
lamps -- 2 cos^3 rad^2 / |c - p|^2, mis_cases.lamp_share's measure -- is at least NEAR_SHARE; the first G = 48 of them, n = 4096 paths each, depth 3.
NEAR_SHARE was found on the CPU (oracle paths, the rule restated by tests/ris_reference.py; test_ris_host.near_share_rows makes the rows) by raising the
share in steps of 0.01 from 0 until the correct rule passes mis_cases' z-test (|mean z| <= 4 / sqrt(G) = 0.577, max |z| <= 5) while control A (r is
dropped from the contribution) and control B (step 7 with q = nl) both fail it.  Recorded before any device ran, as mean z / max |z|:
  share >= 0.00: the correct rule FAILS (6.430 / 82.11): groups whose plain paths never find a lamp have no variance to divide by (A 1.137 / 63.69,
                 B 10.061 / 82.11);
  share >= 0.01: correct  0.071 / 1.81; control A -5.890 /  8.89; control B 6.545 / 8.38   <- NEAR_SHARE
  share >= 0.02: correct -0.106 / 3.14; control A -5.516 / 10.24; control B 6.762 / 9.23
  share >= 0.03: correct  0.097 / 1.85; control A -5.141 /  8.94; control B 7.154 / 9.23
  share >= 0.05: correct  0.036 / 2.07; control A -4.692 / 10.16; control B 7.112 / 9.71
  share >= 0.10: correct  0.015 / 1.48; control A -4.126 /  8.65; control B 7.135 / 9.71
test_ris_host.test_near_share_row asserts the NEAR_SHARE row on the CPU; the GPU test asserts pass, fail and fail on the device's own radiance."""
import functools

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd import hitable as hit
from raytrace_clj_amd import shader as shad
from raytrace_clj_amd import texture as tex
from raytrace_clj_amd import util
from raytrace_clj_amd.util import SplitMix64, vec3
from tests import direct_cases as dcs
from tests import mis_cases as mcs
from tests import nee_cases as ncs

CASES = (("lamps8", "f64"), ("lamps-spheres", "f64"), ("lamps-spheres", "f32"))
ONE_LAMP_CASES, DEPTHS = ncs.CASES, ncs.DEPTHS
NEAR_G, NEAR_N, NEAR_DEPTH = mcs.NEAR_G, mcs.NEAR_N, ncs.ESTIMAND_DEPTH
NEAR_SEED = 0x524953
NEAR_SHARE = 0.01
FRAMES = ((13, 7), (19, 11))  # partial tiles on both axes


def _lamp(*rgb):
    return shad.diffuse_light(tex=tex.constant(color=vec3(*rgb)))


def _camera(nx=dcs.NX, ny=dcs.NY):
    return r.camera.thin_lens_camera(lookfrom=vec3(6, 3, 9), lookat=vec3(0, 1, 0), vup=vec3(0, 1, 0), vfov=35, aspect=float(nx) / float(ny),
                                     aperture=0.0, focus_dist=10.0, t0=0.0, t1=1.0)


def lamps8_scene():
    grey = shad.lambertian(albedo=tex.constant(color=vec3(0.5, 0.5, 0.5)))
    blue = shad.lambertian(albedo=tex.constant(color=vec3(0.1, 0.2, 0.7)))
    warm, cold, green, off = _lamp(5, 4, 3), _lamp(2, 3, 6), _lamp(1, 4, 1), _lamp(0, 0, 0)
    items = [
        hit.sphere(center=vec3(0, -1000, 0), radius=1000, material=grey),
        hit.sphere(center=vec3(0, 1, 0), radius=1, material=blue),
        hit.sphere(center=vec3(1.2, 0.5, 2.0), radius=0.5, material=shad.metal(albedo=tex.constant(color=vec3(0.7, 0.6, 0.5)), fuzz=0.0)),
        hit.sphere(center=vec3(-1.2, 0.5, 2.0), radius=0.5, material=shad.dielectric(ri=1.5)),
        hit.sphere(center=vec3(0.5, 5, 1), radius=1.0, material=warm),
        hit.sphere(center=vec3(-4, 3, -2), radius=0.5, material=off),          # the lamp switched off: lum = 0, never chosen, never a sampled light
        hit.uv_sphere(center=vec3(4, 2.5, -1), radius=0.6, material=cold),
        hit.rect_xy(x0=-2, y0=0.5, x1=0, y1=2, k=-3, material=green),
        hit.rect_xz(x0=-1, z0=2, x1=1, z1=4, k=6, material=cold),
        hit.rect_yz(y0=0.5, z0=-1, y1=2, z1=1, k=-4.5, material=warm),
        hit.sphere(center=vec3(2.5, 0.25, 3.0), radius=0.2, material=green),   # the two small lamps close to the floor
        hit.sphere(center=vec3(-2.5, 0.3, 3.5), radius=0.25, material=warm),
    ]
    return {"camera": _camera(), "world": hit.make_bvh(items, 0.0, 1.0, SplitMix64(0x8A11))}


LOW_LAMPS = ((2.5, 0.25, 3.0, 0.2), (-2.5, 0.3, 3.5, 0.25))  # centre and radius of lamps8's two small lamps


def lamps_spheres_scene():
    return {"camera": _camera(), "world": hit.make_bvh(_sphere_world(), 0.0, 1.0, SplitMix64(0x8A12))}


def _sphere_world():
    grey = shad.lambertian(albedo=tex.constant(color=vec3(0.5, 0.5, 0.5)))
    blue = shad.lambertian(albedo=tex.constant(color=vec3(0.1, 0.2, 0.7)))
    return [
        hit.sphere(center=vec3(0, -1000, 0), radius=1000, material=grey),
        hit.sphere(center=vec3(0, 1, 0), radius=1, material=blue),
        hit.sphere(center=vec3(-2.5, 1, 0.5), radius=1, material=grey),
        hit.sphere(center=vec3(1.2, 0.5, 2.0), radius=0.5, material=shad.metal(albedo=tex.constant(color=vec3(0.7, 0.6, 0.5)), fuzz=0.0)),
        hit.sphere(center=vec3(-1.2, 0.5, 2.0), radius=0.5, material=shad.dielectric(ri=1.5)),
        hit.sphere(center=vec3(0.5, 5, 1), radius=1.5, material=_lamp(5, 4, 3)),
        hit.sphere(center=vec3(3.5, 0.4, 2.5), radius=0.3, material=_lamp(1, 4, 1)),
        hit.sphere(center=vec3(-3.5, 2, 1), radius=0.5, material=_lamp(2, 3, 6)),
        hit.sphere(center=vec3(0, 3, -4), radius=0.7, material=_lamp(0, 0, 0)),
        hit.sphere(center=vec3(2.2, 0.3, 3.5), radius=0.25, material=_lamp(6, 2, 2)),
    ]


def lamps32_scene(n_lamps=32):
    """about 100 small Lambertian spheres on a ground and n_lamps small sphere lamps above and between them"""
    rng = np.random.default_rng(0x32)
    grey = shad.lambertian(albedo=tex.constant(color=vec3(0.5, 0.5, 0.5)))
    items = [hit.sphere(center=vec3(0, -1000, 0), radius=1000, material=grey)]
    for k in range(100):
        x, z, c = rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(0.1, 0.9, 3)
        items.append(hit.sphere(center=vec3(x, 0.2, z), radius=0.2, material=shad.lambertian(albedo=tex.constant(color=vec3(*c)))))
    for k in range(n_lamps):
        x, y, z, c = rng.uniform(-6, 6), rng.uniform(0.6, 2.5), rng.uniform(-6, 6), rng.uniform(0.5, 6.0, 3)
        items.append(hit.sphere(center=vec3(x, y, z), radius=0.15, material=_lamp(*c)))
    return {"camera": _camera(), "world": hit.make_bvh(items, 0.0, 1.0, SplitMix64(0x8A13))}


@functools.lru_cache(maxsize=None)
def lamps32_flat(n_lamps=32):
    return fl.flatten(lamps32_scene(n_lamps))


@functools.lru_cache(maxsize=None)
def flat(name):
    if name == "lamps8":
        from oracle.tree import flatten_with_tree
        return flatten_with_tree(lamps8_scene())
    if name == "lamps-spheres":
        return fl.flatten(lamps_spheres_scene())
    if name == "lamps32":
        return lamps32_flat()
    return dcs.flat(name)


@functools.lru_cache(maxsize=None)
def view_rays(oracle, name):
    """N_POINTS camera rays of the scene through uniform random film points (direct_cases.view_rays' recipe); do not write into them"""
    if name in dcs.SCENES:
        return dcs.view_rays(oracle, name)
    rng = np.random.default_rng(29)
    keys = rng.integers(0, 2 ** 63, dcs.N_POINTS, dtype=np.uint64)
    return np.ascontiguousarray(oracle.probe_camera(flat(name), rng.random((dcs.N_POINTS, 2)), keys)[:, :7])


def records(oracle, f, rays):
    """direct_cases.oracle_records for any flat scene"""
    h = oracle.probe_hit(f, rays, tmin=0.001)
    rec = np.zeros((len(h), dcs.HIT_REC), np.float64)
    rec[:, :11] = h
    found = h[:, 0] != 0.0
    rec[found, 11] = np.asarray(f.prim_mat, np.float64)[h[found, 1].astype(np.int64)]
    return rec


def low_lamp_share(rec):
    """the larger of the two low lamps' shares of the scatter lobe (mis_cases.lamp_share's measure, per lamp)"""
    best = np.zeros(len(rec))
    for cx, cy, cz, rad in LOW_LAMPS:
        to = np.array([cx, cy, cz]) - rec[:, 3:6]
        d2 = (to * to).sum(axis=1)
        with np.errstate(all="ignore"):
            cos = (rec[:, 6:9] * to).sum(axis=1) / np.sqrt(d2 * (rec[:, 6:9] ** 2).sum(axis=1))
            best = np.maximum(best, np.where(cos > 0.0, 2.0 * cos ** 3 * rad ** 2 / d2, 0.0))
    return best


@functools.lru_cache(maxsize=None)
def near_candidates(oracle, count=40000):
    """camera rays of lamps8 through `count` uniform random film points whose first hit is the ground -> (rays [m, 7], share [m]) in film order"""
    f = flat("lamps8")
    rng = np.random.default_rng(NEAR_SEED)
    keys = rng.integers(0, 2 ** 63, count, dtype=np.uint64)
    view = np.ascontiguousarray(oracle.probe_camera(f, rng.random((count, 2)), keys)[:, :7])
    rec = records(oracle, f, view)
    ground = int(np.flatnonzero(np.asarray(f.prim_geom, np.float64).reshape(-1, 9)[:, 3] == 1000.0)[0])
    floor = (rec[:, 0] != 0.0) & (rec[:, 1] == float(ground))
    return view[floor], low_lamp_share(rec[floor])


@functools.lru_cache(maxsize=None)
def near_inputs(oracle, share=None, groups=NEAR_G, n=NEAR_N):
    """-> (rays [groups * n, 7], keys [groups * n]): the first `groups` floor candidates whose low-lamp share is >= share (NEAR_SHARE), each repeated n
    times; path r of group g is keyed sample_key(NEAR_SEED, g, r), what the render calls derive without keys"""
    view, s = near_candidates(oracle)
    chosen = np.flatnonzero(s >= (NEAR_SHARE if share is None else share))[:groups]
    assert len(chosen) == groups, len(chosen)
    rays = np.ascontiguousarray(np.repeat(view[chosen], n, axis=0))
    g, k = (a.ravel() for a in np.meshgrid(np.arange(groups), np.arange(n), indexing="ij"))
    return rays, util.sample_keys(NEAR_SEED, g, k)


# the planar check: mis_cases.PLANAR's vertex at the origin (normal +z) under THREE unoccluded rect_xy lamps of different emission at once
PLANAR3 = tuple((h, rect, le) for (h, rect), le in zip(mcs.PLANAR, ((1.0, 1.0, 1.0), (4.0, 2.0, 1.0), (0.5, 3.0, 2.0))))


def planar3_table():
    return np.concatenate([mcs.planar_table(h, rect) * np.array([1, 1, 1, 1, 1, 1, 1, *le]) for h, rect, le in PLANAR3])
