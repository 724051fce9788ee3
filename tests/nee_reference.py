"""Shared by test_nee_host.py (CPU) and test_gpu_nee.py (GPU): the NEE rule of include/rtmi.h restated in numpy over path logs -- the oracle's
probe_paths logs on the CPU, the device's own on the GPU.  Steps 2 - 4 (light, sample, weight) are camera.nee_samples; step 1 (which vertices), step 5
(the contributions and their fold), step 6 (the closing emission) and step 7 live here.  Nothing here imports the device library.  Not a test module
(pytest collects test_*.py only)."""
import numpy as np

from raytrace_clj_amd import camera as cam
from raytrace_clj_amd import util

SEG_REC, NEE_REC = 12, 24
LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT, TEX_CONSTANT = 0, 1, 2, 3, 0
T_MIN, T_MAX = 0.001, 1.0 - 0.001
INV_PI = float.fromhex("0x1.45f306dc9c883p-2")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def vertices(flat, log, nlog):
    """step 1 -> bool [n, max_seg]: the logged vertices where a Lambertian scatter happened (the log's scattered flag already holds depth > 0)"""
    n, max_seg = log.shape[:2]
    logged = np.arange(max_seg)[None, :] < np.asarray(nlog)[:, None]
    prim = np.where(logged, log[:, :, 0], 0.0).astype(np.int64)
    kind = np.asarray(flat.mat_kind, np.int64)[np.asarray(flat.prim_mat, np.int64)[prim]]
    return logged & (log[:, :, 11] == 1.0) & (kind == LAMBERTIAN)


def samples(log, at, keys, table):
    """steps 2 - 4 at the vertices `at` of paths keyed `keys` -> (path index, vertex index, light, d [m, 3], w [m], built [m]), in path-major order"""
    i, j = np.nonzero(at)
    K = np.asarray(keys, np.uint64)[i]
    ks, kp = util.sample_keys(K, j, np.zeros(len(j), np.int64)), util.sample_keys(K, j, np.ones(len(j), np.int64))
    l, d, w, built = cam.nee_samples(log[i, j, 2:5], log[i, j, 5:8], table, ks, kp)
    return i, j, l, d, w, built


def shadow_rays(log, i, j, d, times):
    """the rays of the built samples: origin p, direction d, the path ray's time"""
    rays = np.zeros((len(i), 7), np.float64)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = log[i, j, 2:5], d, np.asarray(times, np.float64)[i]
    return rays


def attenuations(flat, log, nlog, real=np.float64):
    """T after every logged vertex for scenes whose albedos are Constant textures: the running product, in the call's precision, of the scattered
    vertices' albedos (glass: 1) -> [n, max_seg, 3] float64"""
    n, max_seg = log.shape[:2]
    logged = np.arange(max_seg)[None, :] < np.asarray(nlog)[:, None]
    prim = np.where(logged, log[:, :, 0], 0.0).astype(np.int64)
    mat = np.asarray(flat.prim_mat, np.int64)[prim]
    kind = np.asarray(flat.mat_kind, np.int64)[mat]
    tex = np.asarray(flat.mat_tex, np.int64)[mat]
    assert (np.asarray(flat.tex_kind, np.int64)[tex[logged & (kind != DIELECTRIC)]] == TEX_CONSTANT).all()
    albedo = np.asarray(flat.tex_param, np.float64).reshape(-1, 12)[np.maximum(tex, 0), 0:3].astype(real)
    albedo[kind == DIELECTRIC] = 1.0
    T = np.ones((n, max_seg, 3), real)
    run = np.ones((n, 3), real)
    for k in range(max_seg):
        scat = logged[:, k] & (log[:, k, 11] == 1.0)
        run = np.where(scat[:, None], run * albedo[:, k], run)
        T[:, k] = run
    return T.astype(np.float64)


def fold(n, max_seg, i, j, l, w, free, T, table, lobe_w=None):
    """step 5 -> (contributions [n, max_seg, 3], accum [n, 3]): T * ((Le * w) * nl) where the ray was built and found nothing, added in vertex order
    from +0.0.  lobe_w: other weights in w's place (the negative control)."""
    nl = np.float64(len(table))
    ww = w if lobe_w is None else lobe_w
    contrib = np.zeros((n, max_seg, 3), np.float64)
    contrib[i[free], j[free]] = T[i[free], j[free]] * ((table[l[free], 7:10] * ww[free, None]) * nl)
    accum = np.zeros((n, 3), np.float64)
    for k in range(max_seg):
        accum = accum + contrib[:, k]
    return contrib, accum


def dropped(log, nlog, nseg, at, light_prims):
    """step 6 -> bool [n]: the path ended on a sampled light's primitive (its last segment is logged: a miss logs nothing) and its previous vertex took
    a light sample"""
    nlog, nseg = np.asarray(nlog, np.int64), np.asarray(nseg, np.int64)
    n = len(nlog)
    ended = (nlog == nseg) & (nlog >= 2)
    last = np.maximum(nlog - 1, 0)
    rows = np.arange(n)
    on_light = ended & (log[rows, last, 11] == 0.0) & np.isin(log[rows, last, 0].astype(np.int64), np.asarray(light_prims, np.int64))
    return on_light & at[rows, np.maximum(nlog - 2, 0)]


def cosine_lobe_weights(log, i, j, d, built, table, l):
    """the weight a cosine-weighted scatter would call for, cos cos' area / (pi d^2): the negative control's lobe"""
    n = log[i, j, 5:8]
    n = n / np.sqrt((n * n).sum(axis=1))[:, None]
    d2 = (d * d).sum(axis=1)
    cp = (n * d).sum(axis=1)
    kind = table[l, 0].astype(np.int64)
    sphere = kind <= 1
    q = log[i, j, 2:5] + d
    s = np.where(sphere[:, None], (q - table[l, 1:4]) / np.where(sphere, table[l, 4], 1.0)[:, None],
                 np.stack([kind == 5, kind == 4, kind == 3], axis=1).astype(np.float64))
    cl = np.abs((s * d).sum(axis=1))
    with np.errstate(all="ignore"):
        return np.where(built, ((cp * cl) / (d2 * d2)) * table[l, 6] * INV_PI, 0.0)


def z_scores(plain, nee):
    """per group, on the channel sum: (m_nee - m_plain) / sqrt(v_nee / n + v_plain / n); plain, nee [G, n, 3] radiances"""
    a, b = np.asarray(plain, np.float64).sum(axis=2), np.asarray(nee, np.float64).sum(axis=2)
    n = a.shape[1]
    return (b.mean(axis=1) - a.mean(axis=1)) / np.sqrt(b.var(axis=1, ddof=1) / n + a.var(axis=1, ddof=1) / n)


def same_estimand(z):
    """the issue's two conditions on the z scores of G groups"""
    z = np.asarray(z, np.float64)
    return bool(abs(z.mean()) <= 4.0 / np.sqrt(len(z)) and np.abs(z).max() <= 5.0)


def restate(oracle, flat, rays, keys, depth, lights, ctr0=0, step6=True, cosine=False):
    """The light-sampled radiance of every path, from the oracle's parts: its probe_paths logs and plain radiance, camera.nee_samples, its probe_hit
    over (0.001, 0.999) as the shadow flags, the Constant albedos.  step6 = False keeps every closing emission, cosine = True weighs with the cosine
    lobe: the two negative controls.  No lights: the plain path.  -> (radiance [n, 3], plain radiance [n, 3])"""
    rays, keys = np.ascontiguousarray(rays, np.float64), np.asarray(keys, np.uint64)
    max_seg = depth + 1
    rgb0, nseg, log, nlog = oracle.probe_paths(flat, rays, keys, depth=depth, ctr0=ctr0, max_seg=max_seg)
    if len(lights) == 0:
        return rgb0.copy(), rgb0
    table = cam.light_table(flat, lights)
    at = vertices(flat, log, nlog)
    i, j, l, d, w, built = samples(log, at, keys, table)
    occluded = np.zeros(len(i), bool)
    occluded[built] = oracle.probe_hit(flat, shadow_rays(log, i, j, d, rays[:, 6])[built], tmin=T_MIN, tmax=T_MAX)[:, 0] != 0.0
    T = attenuations(flat, log, nlog)
    other = cosine_lobe_weights(log, i, j, d, built, table, l) if cosine else None
    _, accum = fold(len(rays), max_seg, i, j, l, w, built & ~occluded, T, table, lobe_w=other)
    drop = dropped(log, nlog, nseg, at, lights) if step6 else np.zeros(len(rays), bool)
    return accum + np.where(drop[:, None], 0.0, rgb0), rgb0
