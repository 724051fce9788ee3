"""Shared by test_adaptive_reference.py (CPU) and test_gpu_adaptive.py (GPU): adaptive sampling (rtmi_render_adaptive*) restated with numpy over
the oracle's individual samples (frame_reference.frame_samples) -- Welford's state in sample order, the retirement schedule of a run of
refine_adaptive(first, chunk, cap, eps), the samples every tile ends with, the frame composed tile by tile from in-order folds, and the ray
segments of exactly the samples taken.  Nothing here imports the device library; the oracle is passed in.  Not a test module."""
import numpy as np

import frame_reference as fr

# (scene of frame_reference, precision, (nx, ny), first, chunk, cap, eps): test_adaptive_reference.py holds the conditions these must meet
CASES = [("spheres", "f64", (61, 37), 16, 16, 64, 0.2),
         ("spheres", "f32", (61, 37), 16, 16, 64, 0.2),
         ("mixed", "f64", (61, 37), 16, 16, 64, 0.5),
         ("spheres", "f64", (203, 99), 8, 8, 48, 0.15)]
_samples = {}


def case_id(case):
    name, precision, (nx, ny), first, chunk, cap, eps = case
    return "%s-%s-%dx%d-%d/%d/%d-eps%g" % (name, precision, nx, ny, first, chunk, cap, eps)


def samples(oracle, name, nx, ny, cap):
    """-> (samples [nx, ny, cap, 3] in the oracle's precision, segments [nx, ny, cap]); reference coordinates as frame_samples returns them"""
    key = (oracle.precision, name, nx, ny)
    if key not in _samples or _samples[key][0].shape[2] < cap:
        _samples[key] = fr.frame_samples(oracle, fr.scene(name, nx, ny), nx, ny, cap)
    smp, nseg = _samples[key]
    return smp[:, :, :cap], nseg[:, :, :cap]


def rounds_of(first, chunk, cap):
    """k after every round of refine_adaptive while tiles stay active"""
    ks, k = [], 0
    while k < cap:
        k += min(first if k == 0 else chunk, cap - k)
        ks.append(k)
    return ks


def welford_m2(smp, ks):
    """Welford's M2 of every channel after k samples for every k in ks, in double whatever the frame's precision, updated in sample order with the
    fold kernel's expressions; -> {k: [nx, ny, 3]}"""
    x = smp.astype(np.float64)
    mu, q = x[:, :, 0].copy(), np.zeros(x[:, :, 0].shape)
    out = {1: q.copy()} if 1 in ks else {}
    for s in range(1, max(ks)):
        v = x[:, :, s]
        d = v - mu
        mu = mu + d / float(s + 1)
        q = q + d * (v - mu)
        if s + 1 in ks:
            out[s + 1] = q.copy()
    return out


def stderr_plane(m2, k):
    """out_stderr after k samples: [row, column], the largest channel's sqrt((M2 / (k - 1)) / k); +inf at k = 1"""
    if k == 1:
        return np.full((m2.shape[1], m2.shape[0]), np.inf)
    return fr.to_image(np.sqrt((m2 / float(k - 1)) / float(k))).max(axis=2)


def stderr_two_pass(smp, k):
    return fr.stderr_two_pass(smp, k)


def tile_max(plane, region=None):
    """per 8x8 tile of the frame the largest value of a [row, column] plane over the tile's pixels inside the image and the region; a tile without
    such a pixel holds -inf; NaN propagates.  -> [tiles_y, tiles_x]"""
    ny, nx = plane.shape
    tx, ty = fr.tiles_of(nx, ny)
    pad = np.full((ty * 8, tx * 8), -np.inf)
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    pad[y0:y1, x0:x1] = plane[y0:y1, x0:x1]
    return pad.reshape(ty, 8, tx, 8).max(axis=(1, 3))


def schedule(stderr_of, nx, ny, first, chunk, cap, eps, region=None):
    """The run of refine_adaptive: stderr_of(k) -> the [row, column] noise plane a uniform frame has after k samples.
    -> list over the rounds of (k, n_t [tiles_y, tiles_x] after the round, active [tiles_y, tiles_x] after the round, per-tile maxima of the round);
    it ends like refine_adaptive, at the cap or when no tile is active."""
    tx, ty = fr.tiles_of(nx, ny)
    n_t = np.zeros((ty, tx), np.int64)
    active = np.ones((ty, tx), bool)
    out = []
    for k in rounds_of(first, chunk, cap):
        n_t[active] = k
        worst = tile_max(stderr_of(k), region)
        if k >= 2:
            with np.errstate(invalid="ignore"):
                active = active & ~(worst <= eps)  # retire: every pixel passes se <= eps (a NaN fails)
        out.append((k, n_t.copy(), active.copy(), worst))
        if not active.any():
            break
    return out


def per_pixel(tiles, nx, ny):
    """[tiles_y, tiles_x] -> [row, column]"""
    return np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:ny, :nx]


def compose(frames_of, n_px):
    """the frame in which every pixel comes from the uniform frame with as many samples as the pixel holds: frames_of(n) -> [row, column, ...]"""
    out = None
    for n in np.unique(n_px):
        f = frames_of(int(n))
        out = np.zeros_like(f) if out is None else out
        out[n_px == n] = f[n_px == n]
    return out


def expected_frame(smp, n_px):
    """linear [row, column, 3]: per pixel the in-order fold of its first n samples times 1 / n, in the frame's precision, widened"""
    return compose(lambda n: fr.to_image(fr.mean_of(fr.fold_in_order(smp, 0, n), n)), n_px)


def expected_rays(nseg, n_px):
    """segments of samples [0, n) of every pixel, n = what the pixel's tile holds"""
    seg = np.transpose(nseg, (1, 0, 2))[::-1]  # [row, column, sample]
    taken = np.arange(seg.shape[2])[None, None, :] < n_px[:, :, None]
    return int(seg[taken].sum())


def reference_run(oracle, case):
    """-> (samples, segments, rounds): rounds = schedule(...) of the case from Welford's state of the oracle's samples"""
    name, precision, (nx, ny), first, chunk, cap, eps = case
    assert oracle.precision == precision
    smp, nseg = samples(oracle, name, nx, ny, cap)
    m2 = welford_m2(smp, rounds_of(first, chunk, cap))
    return smp, nseg, schedule(lambda k: stderr_plane(m2[k], k), nx, ny, first, chunk, cap, eps)
