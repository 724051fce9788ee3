"""Shared by test_direct_host.py (CPU) and test_gpu_direct.py (GPU): the scenes of the direct-lighting tests, the view rays their points are
found with, and the facts about those points the GPU tests rely on.  Nothing here imports the device library; the oracle is passed in.  Not a test
module (pytest collects test_*.py only).

Scenes by name:
  "example-light"  scene.make_example_light: a sphere lamp and a rect_xy lamp -- two lights of both kinds, so one wave holds both samplers;
  "cornell"        scene.make_cornell_box: one rect_xz lamp, instanced boxes as occluders (the EXT kernels);
  "two-triangles"  scene.make_two_triangles: every point lies INSIDE its one light, a constant dome of radius 1000 (place() adds the few points whose
                   shadow rays its triangles can occlude);
  "sphere-lamp"    a world of spheres alone (what RTMI_F32 traces) lit by a constant-emission sphere: Lambertian, metal and glass balls on a ground.
View rays: N_POINTS camera rays through uniform random film points (oracle.probe_camera)."""
import functools

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd import hitable as hit
from raytrace_clj_amd import shader as shad
from raytrace_clj_amd import texture as tex
from raytrace_clj_amd.util import SplitMix64, vec3

N_POINTS = 1500  # 23 1/2 waves of points
NX, NY = 40, 24
SCENES = ("example-light", "cornell", "two-triangles", "sphere-lamp")
SPHERE_SCENES = ("sphere-lamp",)
HIT_REC = 12


def sphere_lamp_scene(nx=NX, ny=NY, power=(5.0, 4.0, 3.0), lamp=None):
    """spheres alone: a ground, three Lambertian balls, a metal and a glass one, and the lamp above them (lamp: another record in its place)"""
    rng = SplitMix64(0x11A7)
    grey = shad.lambertian(albedo=tex.constant(color=vec3(0.5, 0.5, 0.5)))
    blue = shad.lambertian(albedo=tex.constant(color=vec3(0.1, 0.2, 0.7)))
    light = shad.diffuse_light(tex=tex.constant(color=vec3(*power)))
    items = [
        hit.sphere(center=vec3(0, -1000, 0), radius=1000, material=grey),
        hit.sphere(center=vec3(0, 1, 0), radius=1, material=blue),
        hit.sphere(center=vec3(-2.5, 1, 0.5), radius=1, material=grey),
        hit.sphere(center=vec3(2.5, 0.7, -0.5), radius=0.7, material=blue),
        hit.sphere(center=vec3(1.2, 0.5, 2.0), radius=0.5, material=shad.metal(albedo=tex.constant(color=vec3(0.7, 0.6, 0.5)), fuzz=0.0)),
        hit.sphere(center=vec3(-1.2, 0.5, 2.0), radius=0.5, material=shad.dielectric(ri=1.5)),
        lamp(light) if lamp else hit.sphere(center=vec3(0.5, 5, 1), radius=1.5, material=light),
    ]
    return {"camera": r.camera.thin_lens_camera(lookfrom=vec3(6, 3, 9), lookat=vec3(0, 1, 0), vup=vec3(0, 1, 0), vfov=35,
                                                aspect=float(nx) / float(ny), aperture=0.0, focus_dist=10.0, t0=0.0, t1=1.0),
            "world": hit.make_bvh(items, 0.0, 1.0, rng)}


def scene(name, **kw):
    if name == "example-light":
        return r.scene.make_example_light(NX, NY)
    if name == "cornell":
        return r.scene.make_cornell_box(NX, NY)
    if name == "two-triangles":
        return r.scene.make_two_triangles(NX, NY)
    assert name == "sphere-lamp", name
    return sphere_lamp_scene(**kw)


@functools.lru_cache(maxsize=None)
def flat(name):
    """the scene flattened, with its nested world for the oracle where the world is more than spheres"""
    if name in SPHERE_SCENES:
        return fl.flatten(scene(name))
    from oracle.tree import flatten_with_tree
    return flatten_with_tree(scene(name))


@functools.lru_cache(maxsize=None)
def view_rays(oracle, name):
    """N_POINTS camera rays of the scene through uniform random film points; do not write into them"""
    rng = np.random.default_rng(29)
    keys = rng.integers(0, 2 ** 63, N_POINTS, dtype=np.uint64)
    return np.ascontiguousarray(oracle.probe_camera(flat(name), rng.random((N_POINTS, 2)), keys)[:, :7])


def oracle_records(oracle, name, rays):
    """the oracle's closest hits of `rays` as rtmi_query_hits' records: probe_hit's eleven values and the hit primitive's material"""
    f = flat(name)
    h = oracle.probe_hit(f, rays, tmin=0.001)
    rec = np.zeros((len(h), HIT_REC), np.float64)
    rec[:, :11] = h
    found = h[:, 0] != 0.0
    rec[found, 11] = np.asarray(f.prim_mat, np.float64)[h[found, 1].astype(np.int64)]
    return rec


PLACED = range(20, 36)  # the rows of the points place() writes


def place(name, hits, view):
    """-> (hits, view) with hand-placed records in rows PLACED where a scene's own first hits cannot occlude a shadow ray.  make_two_triangles: its
    triangles are coplanar, so a ray that leaves one never meets the other, and a ray between two points of the dome (radius 1000) meets a triangle
    (area 1/2) with probability about 1e-7.  The placed points hover in front of the triangles (z < 0: the reference's triangle is hit from that side
    only) and face them: part of the dome is hidden."""
    if name != "two-triangles":
        return hits, view
    hits, view = np.array(hits, np.float64), np.array(view, np.float64)
    f = flat(name)
    for j, row in enumerate(PLACED):
        x, y, prim = (0.25 + 0.01 * j, 0.3, 1) if j % 2 == 0 else (1.3, 1.25 + 0.01 * j, 2)
        z = -(1.5 + 0.05 * j)  # (far enough that the crossing, at t = |z / d.z| with |d| about 1000, lies beyond t-min = 0.001)
        hits[row] = (1.0, float(prim), 1.0, x, y, z, 0.0, 0.0, 1.0, 0.0, 0.0, float(f.prim_mat[prim]))
        view[row] = (x, y, z + 1.0, 0.0, 0.0, -1.0, 0.0)  # seen from the triangles' side: the normal (0, 0, 1) stays
    return hits, view


# ---- eligibility: scenes whose lamp is NOT a light for these calls ---------------------------------------------------------------------------
def not_lights():
    """name -> FlatScene whose only emitter is not eligible (the boundary case is made by hand: a lamp copied behind the world, flagged BOUNDARY)"""
    import copy
    out = {
        "translated": fl.flatten(sphere_lamp_scene(lamp=lambda m: hit.translate(item=hit.sphere(center=vec3(0.5, 4, 1), radius=1.5, material=m), offset=vec3(0, 1, 0)))),
        "moving": fl.flatten(sphere_lamp_scene(lamp=lambda m: hit.moving_sphere(center0=vec3(0.5, 5, 1), t0=0.0, center1=vec3(0.5, 5.5, 1), t1=1.0, radius=1.5, material=m))),
        "zero-extent": fl.flatten(sphere_lamp_scene(lamp=lambda m: hit.rect_xz(x0=1, z0=0, x1=1, z1=2, k=5, material=m))),
        "zero-radius": fl.flatten(sphere_lamp_scene(lamp=lambda m: hit.sphere(center=vec3(0.5, 5, 1), radius=0.0, material=m))),
    }
    f = copy.copy(fl.flatten(sphere_lamp_scene()))
    lamp = len(f.prim_kind) - 1
    f.prim_kind = np.array(f.prim_kind, np.int32)
    f.prim_kind[lamp] |= 16  # RTMI_PRIM_BOUNDARY (the arrays go to the host-only hook, which builds nothing)
    out["boundary"] = f
    return out
