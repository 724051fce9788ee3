"""Shared by test_denoise_reference.py (CPU) and test_gpu_denoise.py (GPU): numpy restatements, written from the text of include/rtmi.h, of
  * the feature pass (rtmi_render_features): every feature sample of a frame composed from the oracle's probes, folded in sample order;
  * the edge-aware filter (rtmi_denoise): one a-trous pass vectorised over the pixels, the taps in the stated order (dy outer, dx inner), every
    operation one IEEE double operation as the header writes it.
Nothing here imports the device library; the oracle is passed in.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

import frame_reference as fr

FEATURES = 8
B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
TINY = 2.0 ** -200  # E of rtmi.h
MAT_DIELECTRIC = 2


# ---- the feature pass ------------------------------------------------------------------------------------------------------------------------
def sample_rays(oracle, flat, nx, ny, na, seed=fr.SEED):
    """the camera ray of every render sample of a pinhole frame, as frame_reference.frame_samples builds them: jitter from draws 0 and 1
    -> (keys [n], rays [n, 7]) in (i, j, s) order, i outermost"""
    assert int(flat.cam_kind) == 0, "a thin lens draws inside get-ray: its samples cannot be rebuilt from the probes"
    R = fr.REAL[oracle.precision]
    ii, jj, ss = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(na), indexing="ij"))
    keys = fr.sample_keys(seed, jj * nx + ii, ss)
    u = (ii.astype(np.float32).astype(R) + fr.draws(keys, 0, oracle.precision)) / R(nx)
    v = (jj.astype(np.float32).astype(R) + fr.draws(keys, 1, oracle.precision)) / R(ny)
    cam = oracle.probe_camera(flat, np.stack([u, v], 1).astype(np.float64), keys)
    assert (cam[:, 7] == 0).all()
    return keys, cam[:, :7]


def albedo_of(oracle, flat, prim, uvp):
    """the material's texture at (u, v, p) for every hit: probe_texture per texture; Dielectric: (1 1 1)"""
    mat = np.asarray(flat.prim_mat)[prim]
    kind, tex = np.asarray(flat.mat_kind)[mat], np.asarray(flat.mat_tex)[mat]
    out = np.ones((len(prim), 3))
    for t in np.unique(tex[kind != MAT_DIELECTRIC]):
        sel = (tex == t) & (kind != MAT_DIELECTRIC)
        out[sel] = oracle.probe_texture(flat, int(t), uvp[sel])
    return out


def _depth(R, p, o):
    e = p.astype(R) - o.astype(R)
    d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    assert d.dtype == R
    return d


def feature_samples(oracle, flat, nx, ny, na, seed=fr.SEED):
    """-> [nx, ny, na, 8] in the oracle's precision, indexed [i, j, s, channel] in reference coordinates: rays from probe_camera, hits from
    probe_hit (t-min 0.001), albedo from probe_texture.  For worlds without media (a medium draws inside hit?: feature_samples_media)."""
    R = fr.REAL[oracle.precision]
    keys, rays = sample_rays(oracle, flat, nx, ny, na, seed)
    hit = oracle.probe_hit(flat, rays)  # hit?, prim, t, p.xyz, normal.xyz, u, v
    f = np.zeros((len(rays), FEATURES), R)
    h = hit[:, 0] != 0
    f[h, 0:3] = albedo_of(oracle, flat, hit[h, 1].astype(np.int64), hit[h][:, [9, 10, 3, 4, 5]])
    f[h, 3:6] = hit[h, 6:9]
    f[h, 6] = _depth(R, hit[h, 3:6], rays[h, 0:3])
    f[h, 7] = 1
    return f.reshape(nx, ny, na, FEATURES)


def feature_samples_media(oracle, flat, nx, ny, na, seed=fr.SEED, depth=fr.DEPTH):
    """the same for a world with media: prim, t, p and normal of segment 0 from probe_paths with the stream continuing at draw 2 (the media draw
    from it); textures of such worlds here are constant, so uv = (0, 0) serves"""
    R = fr.REAL[oracle.precision]
    keys, rays = sample_rays(oracle, flat, nx, ny, na, seed)
    _, _, log, nlog = oracle.probe_paths(flat, rays, keys, depth=depth, ctr0=2, max_seg=1)
    f = np.zeros((len(rays), FEATURES), R)
    h = nlog > 0
    seg = log[h, 0]  # prim, t, p.xyz, n.xyz, ...
    uvp = np.concatenate([np.zeros((len(seg), 2)), seg[:, 2:5]], axis=1)
    f[h, 0:3] = albedo_of(oracle, flat, seg[:, 0].astype(np.int64), uvp)
    f[h, 3:6] = seg[:, 5:8]
    f[h, 6] = _depth(R, seg[:, 2:5], rays[h, 0:3])
    f[h, 7] = 1
    return f.reshape(nx, ny, na, FEATURES)


def feature_frame(smp, na=None):
    """the feature buffers the pass must return for these samples (the first na of them): the frame's fold -- start FROM sample 0, add in order,
    times R(1) / R(na) -- widened; [row, column, 8], row 0 = top"""
    na = smp.shape[2] if na is None else na
    return fr.to_image(fr.mean_of(fr.fold_in_order(smp, 0, na), na))


# ---- the filter ------------------------------------------------------------------------------------------------------------------------------
def _sq3(e):
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def atrous_pass(c, V, feat, step, sigma_c, sigma_n, sigma_a, sigma_d, have_stderr):
    """one pass of rtmi_denoise with tap distance `step`: c [ny, nx, 3], V [ny, nx], feat [ny, nx, 8] or None -> (c', V')"""
    ny, nx, _ = c.shape
    finite = np.isfinite(c).all(axis=2)
    W, S, T = np.zeros((ny, nx)), np.zeros((ny, nx, 3)), np.zeros((ny, nx))
    use_c, use_n = have_stderr and sigma_c > 0, feat is not None and sigma_n > 0
    use_a, use_d = feat is not None and sigma_a > 0, feat is not None and sigma_d > 0
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                y0, y1, x0, x1 = max(0, -oy), min(ny, ny - oy), max(0, -ox), min(nx, nx - ox)
                if y0 >= y1 or x0 >= x1:
                    continue  # every tap of this offset lies outside the image
                P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                take = finite[P] & finite[Q]
                x = np.zeros((y1 - y0, x1 - x0))
                if use_c:
                    x = x + _sq3(c[P] - c[Q]) / ((sigma_c * sigma_c) * (V[P] + V[Q]) + TINY)
                if use_n:
                    x = x + _sq3(feat[P][..., 3:6] - feat[Q][..., 3:6]) / (sigma_n * sigma_n)
                if use_a:
                    x = x + _sq3(feat[P][..., 0:3] - feat[Q][..., 0:3]) / (sigma_a * sigma_a)
                if use_d:
                    dp, dq = feat[P][..., 6], feat[Q][..., 6]
                    e, pp, qq = dp - dq, dp * dp, dq * dq
                    x = x + (e * e) / ((sigma_d * sigma_d) * np.where(qq > pp, qq, pp) + TINY)
                take &= ~np.isnan(x)
                r = 1.0 / (1.0 + x)
                w = (B3[dy + 2] * B3[dx + 2]) * ((r * r) * (r * r))
                take &= w > 0.0
                W[P] = np.where(take, W[P] + w, W[P])
                S[P] = np.where(take[..., None], S[P] + w[..., None] * c[Q], S[P])
                T[P] = np.where(take, T[P] + (w * w) * V[Q], T[P])
        done = W != 0.0
        c2 = np.where(done[..., None], S / W[..., None], c)
        V2 = np.where(done, T / (W * W), V)
    return c2, V2


def denoise(linear, stderr=None, features=None, iterations=5, sigma_c=0.0, sigma_n=0.0, sigma_a=0.0, sigma_d=0.0):
    """rtmi_denoise restated -> (linear, rgb8, stderr)"""
    c = np.array(linear, np.float64)
    if iterations == 0:
        se = np.zeros(c.shape[:2]) if stderr is None else np.array(stderr, np.float64)
        return c, fr.quantise(c), se
    with np.errstate(all="ignore"):
        V = np.zeros(c.shape[:2]) if stderr is None else np.asarray(stderr, np.float64) * np.asarray(stderr, np.float64)
    feat = None if features is None else np.asarray(features, np.float64)
    for i in range(iterations):
        c, V = atrous_pass(c, V, feat, 1 << i, sigma_c, sigma_n, sigma_a, sigma_d, stderr is not None)
    with np.errstate(all="ignore"):
        return c, fr.quantise(c), np.sqrt(V)


def b3_blur(img):
    """the separable B3 blur with border renormalisation: rows then columns of the image and of a plane of ones, then the quotient"""
    def blur1(a, axis):
        out = np.zeros_like(a)
        n = a.shape[axis]
        for d in range(-2, 3):
            lo, hi = max(0, -d), min(n, n - d)
            dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
            dst[axis], src[axis] = slice(lo, hi), slice(lo + d, hi + d)
            out[tuple(dst)] += B3[d + 2] * a[tuple(src)]
        return out
    num = blur1(blur1(np.asarray(img, np.float64), 0), 1)
    den = blur1(blur1(np.ones(img.shape[:2]), 0), 1)
    return num / (den[..., None] if num.ndim == 3 else den)


# ---- inputs for the filter tests: a pure image operation needs no scene --------------------------------------------------------------------------
def synthetic_frame(nx, ny, seed=0):
    """a noisy frame with edges, its noise estimate and feature buffers that mark some of the edges -> (linear, stderr, features)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    region = ((xx * 3 // nx) + 3 * (yy * 2 // ny)).astype(np.int64)  # six flat regions
    base = rng.random((6, 3))[region] * (0.5 + 0.5 * np.sin(xx / 7.0)[..., None] ** 2)
    se = 0.02 + 0.2 * rng.random((ny, nx)) * base.mean(axis=2)
    lin = base + se[..., None] * rng.normal(size=(ny, nx, 3))
    ft = np.zeros((ny, nx, FEATURES))
    ft[..., 0:3] = rng.random((6, 3))[region] + 0.01 * rng.normal(size=(ny, nx, 3))
    nrm = rng.normal(size=(6, 3))[region] + 0.05 * rng.normal(size=(ny, nx, 3))
    ft[..., 3:6] = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
    ft[..., 6] = 5.0 + region + 0.02 * xx + 0.01 * rng.random((ny, nx))
    ft[..., 7] = 1.0
    return np.ascontiguousarray(lin), np.ascontiguousarray(se), np.ascontiguousarray(ft)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
