"""Shared by test_direct_host.py (CPU) and test_gpu_direct.py (GPU): numpy restatements of what rtmi_direct_irradiance* and rtmi_render_direct* compute,
written from the text of include/rtmi.h ("the lights", "the light rule", "the fold", rtmi_render_direct's resolve).  Step 1 (which points yield a ray,
which side, which time, lambert_only), the contributions, the fold and the resolve live here; steps 2 - 6 are camera.light_samples.  Nothing here imports
the device library.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

from raytrace_clj_amd import camera as cam
from tests import occlusion_reference as occ

HIT_REC, DIRECT_REC = 12, 4
SEED = 0x5EED0002
INV_PI = float.fromhex("0x1.45f306dc9c883p-2")
SPHERE, UVSPHERE, RECT_XY, RECT_XZ, RECT_YZ, BOUNDARY = 0, 1, 3, 4, 5, 16
LAMBERTIAN, DIFFUSE_LIGHT, TEX_CONSTANT = 0, 3, 0


def eligible(flat):
    """the header's eligibility rule over a FlatScene -> primitive indices in primitive order"""
    out = []
    geom = np.asarray(flat.prim_geom, np.float64).reshape(-1, 9)
    chains = np.asarray(getattr(flat, "prim_xform", np.zeros((len(geom), 2))), np.int64).reshape(-1, 2)
    for i, kind in enumerate(np.asarray(flat.prim_kind, np.int64)):
        g = geom[i]
        if kind in (SPHERE, UVSPHERE):
            shape = g[3] > 0.0
        elif kind in (RECT_XY, RECT_XZ, RECT_YZ):
            shape = g[2] - g[0] != 0.0 and g[3] - g[1] != 0.0
        else:
            shape = False  # a boundary primitive carries BOUNDARY in its kind and ends here too
        m = int(flat.prim_mat[i])
        if shape and chains[i, 1] == 0 and flat.mat_kind[m] == DIFFUSE_LIGHT and flat.tex_kind[int(flat.mat_tex[m])] == TEX_CONSTANT:
            out.append(i)
    return np.asarray(out, np.int32)


def light_items(hits, lights, n_samples, view=None, first=0, seed=SEED, time=0.0, lambert_only=False, mat_kind=None):
    """-> (rays [items, 7], weights [items], built [items]): item (g * n_samples + k) * n_lights + l; zeros where no ray is built"""
    hits, view = occ._records(hits, view)
    lights = np.asarray(lights, np.float64).reshape(-1, cam.LIGHT_REC)
    ok = occ.yields_a_ray(hits)
    if lambert_only:
        mat_kind = np.asarray(mat_kind, np.int64)
        with np.errstate(all="ignore"):
            known = ok & (hits[:, 11] >= 0.0) & (hits[:, 11] < float(len(mat_kind)))
        index = np.where(known, hits[:, 11], 0.0).astype(np.int64)
        ok = known & (mat_kind[index] == LAMBERTIAN)
    p, n = hits[:, 3:6].copy(), hits[:, 6:9].copy()
    if view is not None:  # the side the viewer is on
        with np.errstate(all="ignore"):
            away = occ._dot3(n, view[:, 3:6]) > 0.0
        n[away] = -n[away]
    p[~ok], n[~ok] = 0.0, (0.0, 1.0, 0.0)  # (every point keeps its index g, which keys its streams; these items are zeroed below)
    rays, w, built = cam.light_samples(p, n, lights, n_samples, first=first, seed=seed)
    per_point = int(n_samples) * len(lights)
    built &= np.repeat(ok, per_point)
    rays[:, 6] = np.repeat(view[:, 6], per_point) if view is not None else float(time)
    rays[~built] = 0.0
    return rays, np.where(built, w, 0.0), built


def contributions(weights, built, flags, lights):
    """step 7: Le * w per channel where the ray was built and is not occluded, else +0.0 -> [items, 3]"""
    lights = np.asarray(lights, np.float64).reshape(-1, cam.LIGHT_REC)
    le = lights[np.arange(len(weights)) % len(lights), 7:10]
    lit = built & (np.asarray(flags) == 0)
    return np.where(lit[:, None], le * weights[:, None], 0.0)


def fold(contrib, n_points, n_samples, first=0, state=None):
    """the in-order sum of every point's items, starting FROM the first item, then E = sum * (1 / samples) -> (E [n_points, 3], state)"""
    contrib = np.asarray(contrib, np.float64).reshape(n_points, -1, 3)
    if state is not None and first > 0:
        acc, start = np.array(state[:, 0:3]), 0
    else:
        acc, start, first = contrib[:, 0].copy(), 1, 0
    for i in range(start, contrib.shape[1]):
        acc = acc + contrib[:, i]
    samples = first + int(n_samples)
    new_state = np.concatenate([acc, np.full((n_points, 1), float(samples))], axis=1)
    return acc * (1.0 / float(samples)), new_state


def resolve(hits, E, mat_kind, texture):
    """rtmi_render_direct's resolve: texture [n, 3] = the material's texture at every record (probe_texture), anything for misses"""
    hits = np.asarray(hits, np.float64).reshape(-1, HIT_REC)
    mat_kind = np.asarray(mat_kind, np.int64)
    hit = hits[:, 0] != 0.0
    kind = np.where(hit, mat_kind[np.where(hit, hits[:, 11], 0.0).astype(np.int64)], -1)
    out = np.zeros((len(hits), 3), np.float64)
    emit, lamb = kind == DIFFUSE_LIGHT, kind == LAMBERTIAN
    out[emit] = texture[emit]
    out[lamb] = (texture[lamb] * E[lamb]) * INV_PI
    return out
