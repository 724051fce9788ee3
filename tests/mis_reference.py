"""Shared by test_mis_host.py (CPU) and test_gpu_mis.py (GPU): the MIS rule of include/rtmi.h restated in numpy over path logs -- the oracle's
probe_paths logs on the CPU, the device's own on the GPU.  Step 2 (the pick) is camera.mis_pick, step 3 camera.nee_samples with that pick, step 4
camera.mis_weight, step 6 camera.mis_lobe, step 7 camera.mis_closing; which vertices, the fold and the closing emission's bookkeeping live here, on top
of tests/nee_reference.py (imported, not edited).  Nothing here imports the device library.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import util
from tests import nee_reference as nref

MIS_REC = 28
bits = nref.bits


def samples(log, at, keys, table, light_choice):
    """steps 2 - 4 and 6 at the vertices `at` -> dict: i, j (path, vertex), l, d, w, built, x, m, g per light-sampled vertex in path-major order, and
    q [nl], live [nl] of the pick"""
    i, j = np.nonzero(at)
    K = np.asarray(keys, np.uint64)[i]
    ks, kp = util.sample_keys(K, j, np.zeros(len(j), np.int64)), util.sample_keys(K, j, np.ones(len(j), np.int64))
    l, q, live = cam.mis_pick(table, kp, light_choice)
    l, d, w, built = cam.nee_samples(log[i, j, 2:5], log[i, j, 5:8], table, ks, kp, light=l)
    x, m = cam.mis_weight(w, q[l])
    g = cam.mis_lobe(log[i, j, 5:8], log[i, j, 8:11], points=log[i, j, 2:5])
    return dict(i=i, j=j, l=l, d=d, w=w, built=built, x=x, m=m, g=g, q=q, live=live)


def fold(n, max_seg, s, free, T, table):
    """step 5 -> (contributions [n, max_seg, 3], accum [n, 3]): T * (Le * m) where the ray was built and found nothing, added in vertex order from +0.0"""
    i, j, l, m = s["i"], s["j"], s["l"], s["m"]
    contrib = np.zeros((n, max_seg, 3), np.float64)
    contrib[i[free], j[free]] = T[i[free], j[free]] * (table[l[free], 7:10] * m[free, None])
    accum = np.zeros((n, 3), np.float64)
    for k in range(max_seg):
        accum = accum + contrib[:, k]
    return contrib, accum


def closing(log, nlog, nseg, at, lights, s, table):
    """step 7 -> (weighted bool [n], x' [n] (0 where not weighted), m' [n] (1 where not weighted)).  weighted: where the NEE rule drops the closing emission,
    the lights by power with omega = 0 not counting as sampled lights; l' = the emitter's first index among the lights that count."""
    lights = np.asarray(lights, np.int64)
    listed = np.where(s["live"], lights, -1)
    weighted = nref.dropped(log, nlog, nseg, at, listed[listed >= 0])
    n = len(weighted)
    rows = np.flatnonzero(weighted)
    nlog = np.asarray(nlog, np.int64)
    last, prev = nlog[rows] - 1, nlog[rows] - 2
    lp = (log[rows, last, 0].astype(np.int64)[:, None] == listed[None, :]).argmax(axis=1)
    g_at = np.zeros(at.shape, np.float64)
    g_at[s["i"], s["j"]] = s["g"]
    xq, mq = cam.mis_closing(g_at[rows, prev], log[rows, last, 5:8], log[rows, prev, 8:11], log[rows, last, 1], table[lp, 6], s["q"][lp])
    x, m = np.zeros(n, np.float64), np.ones(n, np.float64)
    x[rows], m[rows] = xq, mq
    return weighted, x, m


def restate(oracle, flat, rays, keys, depth, lights, light_choice=0, ctr0=0, control=None):
    """The MIS radiance of every path from the oracle's parts, as nee_reference.restate: its probe_paths logs and plain radiance (= the closing emission),
    its probe_hit over (0.001, 0.999) as the shadow flags, the Constant albedos.  control "A": the weighted closing emissions are dropped instead;
    control "B": they are kept whole -- the two wrong rules.  No lights: the plain path.  -> (radiance [n, 3], plain radiance [n, 3], the samples' dict)"""
    rays, keys = np.ascontiguousarray(rays, np.float64), np.asarray(keys, np.uint64)
    max_seg = depth + 1
    rgb0, nseg, log, nlog = oracle.probe_paths(flat, rays, keys, depth=depth, ctr0=ctr0, max_seg=max_seg)
    if len(lights) == 0:
        return rgb0.copy(), rgb0, None
    table = cam.light_table(flat, lights)
    at = nref.vertices(flat, log, nlog)
    s = samples(log, at, keys, table, light_choice)
    built = s["built"]
    occluded = np.zeros(len(built), bool)
    occluded[built] = oracle.probe_hit(flat, nref.shadow_rays(log, s["i"], s["j"], s["d"], rays[:, 6])[built], tmin=nref.T_MIN, tmax=nref.T_MAX)[:, 0] != 0.0
    T = nref.attenuations(flat, log, nlog)
    contrib, accum = fold(len(rays), max_seg, s, built & ~occluded, T, table)
    weighted, x, m = closing(log, nlog, nseg, at, lights, s, table)
    if control == "A":
        m = np.where(weighted, 0.0, 1.0)
    elif control == "B":
        m = np.ones(len(rays))
    s.update(contrib=contrib, T=T, weighted=weighted, xq=x, mq=m, free=built & ~occluded)
    return accum + rgb0 * m[:, None], rgb0, s
