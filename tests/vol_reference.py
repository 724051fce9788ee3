"""Shared by test_vol_host.py (CPU) and test_gpu_vol.py (GPU): the volume rule of include/rtmi.h restated in numpy over path logs -- the oracle's
probe_paths logs on the CPU, the device's own on the GPU.  Steps 2 and 3 are camera.vol_samples, step 5 camera.vol_lobe, the MIS weights
camera.mis_weight and mis_closing; which vertices, the shadow rays with their keys and times, the folds and the closing emission live here, on top of
tests/nee_reference.py and tests/mis_reference.py (imported, not edited).  Nothing here imports the device library.  Not a test module."""
import numpy as np

from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import util
from tests import mis_reference as mref
from tests import nee_reference as nref

VOL_REC = 29
ISOTROPIC = 4
bits = nref.bits


def vertices(flat, log, nlog):
    """step 1 -> (at, iso) bool [n, max_seg]: the logged vertices where a Lambertian or an Isotropic scatter happened, and the Isotropic ones among them"""
    n, max_seg = log.shape[:2]
    logged = np.arange(max_seg)[None, :] < np.asarray(nlog)[:, None]
    prim = np.where(logged, log[:, :, 0], 0.0).astype(np.int64)
    kind = np.asarray(flat.mat_kind, np.int64)[np.asarray(flat.prim_mat, np.int64)[prim]]
    scat = logged & (log[:, :, 11] == 1.0)
    return scat & ((kind == nref.LAMBERTIAN) | (kind == ISOTROPIC)), scat & (kind == ISOTROPIC)


def times(log, iso, ray_times):
    """the scattered ray's time behind every logged vertex [n, max_seg]: the path ray's, until an Isotropic scatter sets it to the hit's t"""
    n, max_seg = log.shape[:2]
    out = np.zeros((n, max_seg), np.float64)
    run = np.asarray(ray_times, np.float64).copy()
    for k in range(max_seg):
        run = np.where(iso[:, k], log[:, k, 1], run)
        out[:, k] = run
    return out


def samples(log, at, iso, keys, table, estimator, light_choice=0):
    """steps 2, 3 and 5 (and the MIS rule's 2 and 4) at the vertices `at` -> dict per light-sampled vertex in path-major order: i, j, iso, l, d, w, built,
    x, m, g (zeros under the NEE rule), key = the shadow ray's stream key, and q [nl], live [nl] of the pick"""
    i, j = np.nonzero(at)
    K = np.asarray(keys, np.uint64)[i]
    ks, kp, kshadow = (util.sample_keys(K, j, np.full(len(j), c, np.int64)) for c in (0, 1, 2))
    nl = len(table)
    if estimator == 2:
        pick, q, live = cam.mis_pick(table, kp, light_choice)
    else:
        pick, q, live = None, np.full(nl, np.float64(nl)), np.ones(nl, bool)
    l, d, w, built = cam.vol_samples(log[i, j, 2:5], log[i, j, 5:8], iso[i, j], table, ks, kp, light=pick)
    zero = np.zeros(len(i))
    x, m, g = zero, zero, zero
    if estimator == 2:
        x, m = cam.mis_weight(w, q[l])
        g = cam.vol_lobe(log[i, j, 5:8], log[i, j, 8:11], iso[i, j], points=log[i, j, 2:5])
    return dict(i=i, j=j, iso=iso[i, j], l=l, d=d, w=w, built=built, x=x, m=m, g=g, q=q, live=live, key=kshadow)


def shadow_rays(log, s, tm):
    """the rays of all the samples (the unbuilt rows are dropped by the caller): origin p, direction d, the scattered ray's time"""
    i, j = s["i"], s["j"]
    rays = np.zeros((len(i), 7), np.float64)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = log[i, j, 2:5], s["d"], tm[i, j]
    return rays


def fold(n, max_seg, s, free, T, table, estimator):
    """step 4's contributions -> (contributions [n, max_seg, 3], accum [n, 3]): the NEE rule's T * ((Le * w) * nl) or the MIS rule's T * (Le * m)"""
    if estimator == 2:
        return mref.fold(n, max_seg, s, free, T, table)
    return nref.fold(n, max_seg, s["i"], s["j"], s["l"], s["w"], free, T, table)


def closing(log, nlog, nseg, at, lights, s, table, estimator):
    """step 6 -> (weighted or dropped bool [n], x' [n], the factor m' on the closing emission [n]): the NEE rule's 0.0 / 1.0 or the MIS rule's step 7"""
    if estimator == 2:
        return mref.closing(log, nlog, nseg, at, lights, s, table)
    drop = nref.dropped(log, nlog, nseg, at, lights)
    return drop, np.zeros(len(drop)), np.where(drop, 0.0, 1.0)


def restate(oracle, flat, rays, keys, depth, lights, estimator, light_choice=0, shadow_flat=None, keep_after_iso=False):
    """The volume rule's radiance of every path from the oracle's parts: its probe_paths logs and plain radiance (= the closing emission), vol_samples,
    the shadow flags from its probe_paths on the shadow rays with their own keys (depth 0, one segment: "hit with t < 0.999" -- valid where no medium
    reaches the far end of the interval), the Constant albedos, the fold.  shadow_flat: another scene for the shadow rays (control: the media removed);
    keep_after_iso: the closing emission is kept whole behind an Isotropic light sample (control: double counting).
    -> (radiance [n, 3], plain radiance [n, 3], the samples' dict)"""
    rays, keys = np.ascontiguousarray(rays, np.float64), np.asarray(keys, np.uint64)
    max_seg = depth + 1
    rgb0, nseg, log, nlog = oracle.probe_paths(flat, rays, keys, depth=depth, ctr0=0, max_seg=max_seg)
    table = cam.light_table(flat, lights)
    at, iso = vertices(flat, log, nlog)
    s = samples(log, at, iso, keys, table, estimator, light_choice)
    built = s["built"]
    shadow = shadow_rays(log, s, times(log, iso, rays[:, 6]))[built]
    _, _, slog, snlog = oracle.probe_paths(shadow_flat if shadow_flat is not None else flat, shadow, s["key"][built], depth=0, ctr0=0, max_seg=1)
    occluded = np.zeros(len(built), bool)
    occluded[built] = (snlog == 1) & (slog[:, 0, 1] < nref.T_MAX)
    T = nref.attenuations(flat, log, nlog)
    contrib, accum = fold(len(rays), max_seg, s, built & ~occluded, T, table, estimator)
    weighted, x, m = closing(log, nlog, nseg, at, lights, s, table, estimator)
    if keep_after_iso:
        rows = np.arange(len(rays))
        m = np.where(weighted & iso[rows, np.maximum(np.asarray(nlog, np.int64) - 2, 0)], 1.0, m)
    s.update(free=built & ~occluded, occluded=occluded, weighted=weighted, mq=m, at=at, iso_at=iso)
    return accum + rgb0 * m[:, None], rgb0, s
