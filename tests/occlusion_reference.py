"""Shared by test_occlusion_host.py (CPU) and test_gpu_occlusion.py (GPU): numpy restatements of the rays rtmi_occlusion_hemisphere* and
rtmi_occlusion_targets* generate on the device, written from the text of include/rtmi.h ("the hemisphere rule", "the targets rule").  Steps 1 and 2
(which points yield a ray, which side of the surface, which time) and the targets rule live here; steps 3 - 7 are camera.hemisphere_rays_disk.
Nothing here imports the device library.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

from raytrace_clj_amd import camera as cam

HIT_REC = 12
SEED = 0x5EED0002


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _records(hits, view):
    hits = np.asarray(hits, np.float64).reshape(-1, HIT_REC)
    if view is not None:
        view = np.asarray(view, np.float64).reshape(-1, 7)
        assert len(view) == len(hits)
    return hits, view


def yields_a_ray(hits, normal=True):
    """step 1: rec[0] != 0, p (and the normal, where it is read) finite, dot3(n, n) > 0 -> bool [n_points]"""
    hits = np.asarray(hits, np.float64).reshape(-1, HIT_REC)
    ok = (hits[:, 0] != 0.0) & np.isfinite(hits[:, 3:6]).all(axis=1)
    if normal:
        with np.errstate(all="ignore"):
            ok &= np.isfinite(hits[:, 6:9]).all(axis=1) & (_dot3(hits[:, 6:9], hits[:, 6:9]) > 0.0)
    return ok


def _finish(rays, ok, per_point, view, time):
    rays[:, 6] = np.repeat(view[:, 6], per_point) if view is not None else float(time)
    rays[~np.repeat(ok, per_point)] = 0.0  # a point that yields no ray: rows of zeros
    return rays, ok


def hemisphere(hits, n_dirs, view=None, first=0, seed=SEED, time=0.0):
    """-> (rays [n_points * n_dirs, 7], ok [n_points]): row g * n_dirs + k is direction first + k of point g; zeros where ok[g] is False"""
    hits, view = _records(hits, view)
    ok = yields_a_ray(hits)
    p, n = hits[:, 3:6].copy(), hits[:, 6:9].copy()
    if view is not None:  # step 2: the side the viewer is on
        with np.errstate(all="ignore"):
            away = _dot3(n, view[:, 3:6]) > 0.0
        n[away] = -n[away]
    p[~ok], n[~ok] = 0.0, (0.0, 1.0, 0.0)  # (every point keeps its index g, which keys its streams; these rows are zeroed below)
    rays = cam.hemisphere_rays_disk(p, n, n_dirs, first=first, seed=seed)
    return _finish(rays, ok, int(n_dirs), view, time)


def targets(hits, targets, view=None, time=0.0):
    """-> (rays [n_points * n_targets, 7], ok [n_points]): row g * n_targets + k runs from point g towards targets[k]"""
    hits, view = _records(hits, view)
    targets = np.asarray(targets, np.float64).reshape(-1, 3)
    ok = yields_a_ray(hits, normal=False)
    n, k = len(hits), len(targets)
    p = np.repeat(hits[:, 3:6], k, axis=0)
    rays = np.zeros((n * k, 7), np.float64)
    rays[:, 0:3] = p
    with np.errstate(all="ignore"):
        rays[:, 3:6] = np.tile(targets, (n, 1)) - p
    return _finish(rays, ok, k, view, time)


def degenerate(hits):
    """a copy of `hits` with records that yield no ray scattered over it, so that idle lanes sit in the middle of waves: misses, a non-finite
    point, a zero normal, a non-finite normal.  -> (hits, the indices touched)"""
    hits = np.array(hits, np.float64).reshape(-1, HIT_REC)
    n = len(hits)
    idx = [i for i in (7, 64, 65, 66, 100, 200, 300, n - 1) if 0 <= i < n]
    for i in idx:
        hits[i, 0] = 1.0
    for i in idx[:4] + idx[7:]:
        hits[i] = 0.0
    if len(idx) > 4:
        hits[idx[4], 4] = np.nan
    if len(idx) > 5:
        hits[idx[5], 6:9] = 0.0
    if len(idx) > 6:
        hits[idx[6], 7] = np.inf
    return hits, idx
