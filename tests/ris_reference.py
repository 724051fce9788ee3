"""Shared by test_ris_host.py (CPU) and test_gpu_ris.py (GPU): the proposal rule of include/rtmi.h restated in numpy over path logs -- the oracle's
probe_paths logs on the CPU, the device's own on the GPU.  Step 2 (the candidates) is camera.ris_candidates, step 3 (the choice) camera.ris_choose, steps
6 and 7 camera.mis_lobe and mis_closing through tests/mis_reference.py with q = 1; which vertices, the fold and the closing emission's bookkeeping are
nee_reference's and mis_reference's (imported, not edited).  Nothing here imports the device library.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

from raytrace_clj_amd import camera as cam
from tests import mis_reference as mref
from tests import nee_reference as nref

RIS_REC = 32
bits = nref.bits


def samples(log, at, keys, table, control=None):
    """steps 2, 3 and 6 at the vertices `at` -> dict: i, j (path, vertex), l, d, w, x, m of the chosen candidate (zeros where no candidate is live),
    built, g, S, what, r, count per light-sampled vertex in path-major order; q [nl] and live [nl] (lum > 0) for step 7; lum [nl].
    control "B": step 7 with q = nl, the uniform pick's factor -- a wrong neighbour"""
    i, j = np.nonzero(at)
    K = np.asarray(keys, np.uint64)[i]
    nl = len(table)
    d_all, w_all, m_all, what, live, lum = cam.ris_candidates(log[i, j, 2:5], log[i, j, 5:8], table, K, j)
    l, S, sel_what, r, count = cam.ris_choose(what, live, K, j)
    built, a = count > 0, np.arange(len(i))
    d = np.where(built[:, None], d_all[a, l], 0.0)
    w, m = np.where(built, w_all[a, l], 0.0), np.where(built, m_all[a, l], 0.0)
    g = cam.mis_lobe(log[i, j, 5:8], log[i, j, 8:11], points=log[i, j, 2:5])
    q = np.full(nl, np.float64(nl) if control == "B" else 1.0)
    return dict(i=i, j=j, l=l, d=d, w=w, built=built, x=w, m=m, g=g, S=S, what=sel_what, r=r, count=count, q=q, live=lum > 0.0, lum=lum)


def fold(n, max_seg, s, free, T, table, control=None):
    """step 5 -> (contributions [n, max_seg, 3], accum [n, 3]): T * ((Le * m) * r) where the ray was built and found nothing, added in vertex order from
    +0.0.  control "A": r is dropped -- the other wrong neighbour"""
    i, j, l, m = s["i"], s["j"], s["l"], s["m"]
    r = np.ones(len(i)) if control == "A" else s["r"]
    contrib = np.zeros((n, max_seg, 3), np.float64)
    contrib[i[free], j[free]] = T[i[free], j[free]] * ((table[l[free], 7:10] * m[free, None]) * r[free, None])
    accum = np.zeros((n, 3), np.float64)
    for k in range(max_seg):
        accum = accum + contrib[:, k]
    return contrib, accum


def bound(s, T, table):
    """the rule's bound per light-sampled vertex and channel: T.c * (Le_sel.c / lum_sel) * sum_k lum_k (rows of vertices without a live candidate: 0)"""
    total = s["lum"][s["lum"] > 0.0].sum()
    with np.errstate(all="ignore"):
        b = T[s["i"], s["j"]] * (table[s["l"], 7:10] / s["lum"][s["l"]][:, None]) * total
    return np.where(s["built"][:, None], b, 0.0)


closing = mref.closing  # step 7: the MIS rule's, reading q (ones) and live (lum > 0) from the samples' dict


def restate(oracle, flat, rays, keys, depth, lights, ctr0=0, control=None):
    """The radiance of every path under the proposal rule from the oracle's parts, as mis_reference.restate: its probe_paths logs and plain radiance (= the
    closing emission), its probe_hit over (0.001, 0.999) as the shadow flags, the Constant albedos.  No lights: the plain path.
    -> (radiance [n, 3], plain radiance [n, 3], the samples' dict)"""
    rays, keys = np.ascontiguousarray(rays, np.float64), np.asarray(keys, np.uint64)
    max_seg = depth + 1
    rgb0, nseg, log, nlog = oracle.probe_paths(flat, rays, keys, depth=depth, ctr0=ctr0, max_seg=max_seg)
    if len(lights) == 0:
        return rgb0.copy(), rgb0, None
    table = cam.light_table(flat, lights)
    at = nref.vertices(flat, log, nlog)
    s = samples(log, at, keys, table, control)
    built = s["built"]
    occluded = np.zeros(len(built), bool)
    if built.any():
        occluded[built] = oracle.probe_hit(flat, nref.shadow_rays(log, s["i"], s["j"], s["d"], rays[:, 6])[built], tmin=nref.T_MIN, tmax=nref.T_MAX)[:, 0] != 0.0
    T = nref.attenuations(flat, log, nlog)
    contrib, accum = fold(len(rays), max_seg, s, built & ~occluded, T, table, control)
    weighted, x, m = closing(log, nlog, nseg, at, lights, s, table)
    s.update(contrib=contrib, T=T, weighted=weighted, xq=x, mq=m, free=built & ~occluded, at=at)
    return accum + rgb0 * m[:, None], rgb0, s
