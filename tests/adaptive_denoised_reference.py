"""Shared by test_adaptive_denoised_reference.py (CPU) and test_gpu_adaptive_denoised.py (GPU): retirement by a caller's noise map
(rtmi_adaptive_retire*) and the driver that closes the loop between adaptive sampling and the denoiser (refine_adaptive_denoised), restated with
numpy from the text of include/rtmi.h on top of adaptive_reference and denoise_reference.  The model is the sequential schedule: per round the
active tiles get n_t = k, the frame and its standard error are composed per pixel from n_t, the raw rule at eps 0 retires tiles whose samples
are all equal (k >= 2), the frame is filtered, and the tiles whose filtered standard error passes eps retire.  Nothing here imports the device
library; the oracle is passed in.  Not a test module."""
import numpy as np

import adaptive_reference as ar
import denoise_reference as dr
import frame_reference as fr

NA = 4  # feature samples
FILTER = dict(iterations=5, sigma_c=4.0, sigma_n=0.5, sigma_a=0.2, sigma_d=0.2)  # the library's defaults (test_adaptive_denoised_reference.py checks)

# (scene of frame_reference, precision, (nx, ny), first, chunk, cap, eps): test_adaptive_denoised_reference.py holds the conditions these must meet
CASES = [("spheres", "f64", (61, 37), 16, 16, 64, 0.2),
         ("spheres", "f32", (61, 37), 16, 16, 64, 0.2),
         ("mixed", "f64", (61, 37), 16, 16, 64, 0.1),
         ("spheres", "f64", (203, 99), 8, 8, 48, 0.15)]
REGION = (37, 21, 101, 59)  # of the 203 x 99 frame: it cuts tiles on all four sides
_features, _runs = {}, {}


def retire(active, noise, eps, region=None):
    """rtmi_adaptive_retire: active [tiles_y, tiles_x] bool, noise [ny, nx] of the whole frame -> active afterwards.  An active tile retires if
    every pixel of it inside the image and the region passes noise <= eps, compared exactly so: a NaN and +inf fail, -inf passes."""
    worst = ar.tile_max(noise, region)  # NaN propagates through the maximum
    with np.errstate(invalid="ignore"):
        return active & ~(worst <= eps)


def local_tiles(nx, ny, region=None):
    """[tiles_y, tiles_x] bool: the tiles of the frame, those that meet the region"""
    tx, ty = fr.tiles_of(nx, ny)
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    local = np.zeros((ty, tx), bool)
    local[y0 // 8:(y1 + 7) // 8, x0 // 8:(x1 + 7) // 8] = True
    return local


def features(oracle, name, nx, ny, na=NA):
    key = (oracle.precision, name, nx, ny, na)
    if key not in _features:
        _features[key] = dr.feature_frame(dr.feature_samples(oracle, fr.scene(name, nx, ny), nx, ny, na))
    return _features[key]


def schedule(frame_of, stderr_of, feat, nx, ny, first, chunk, cap, eps, flt=FILTER):
    """The run of refine_adaptive_denoised: frame_of(n_px) -> linear [row, column, 3] of the frame whose pixels hold n_px samples,
    stderr_of(k) -> the noise plane a uniform frame has after k samples.
    -> list over the rounds of dicts: k, n_t and active [tiles_y, tiles_x] after the round, linear / stderr of the unfiltered frame, flt_linear /
    flt_rgb8 / flt_stderr of the filtered one, equal = the tiles the all-equal rule retired in this round."""
    tx, ty = fr.tiles_of(nx, ny)
    n_t = np.zeros((ty, tx), np.int64)
    active = np.ones((ty, tx), bool)
    out = []
    for k in ar.rounds_of(first, chunk, cap):
        n_t[active] = k
        n_px = ar.per_pixel(n_t, nx, ny)
        lin, raw = frame_of(n_px), ar.compose(stderr_of, n_px)
        equal = np.zeros_like(active)
        if k >= 2:  # render_adaptive(..., eps = 0): only tiles whose samples are all equal
            equal = active & (ar.tile_max(raw) <= 0.0)
            active = active & ~equal
        f_lin, f_q, f_err = dr.denoise(lin, raw, feat, **flt)
        active = retire(active, f_err, eps)
        out.append(dict(k=k, n_t=n_t.copy(), active=active.copy(), linear=lin, stderr=raw, flt_linear=f_lin, flt_rgb8=f_q, flt_stderr=f_err,
                        equal=equal))
        if not active.any():
            break
    return out


def reference_run(oracle, case):
    """-> (samples, segments, features, rounds) of a case from the oracle's individual samples (kept: the CPU and the GPU test share them)"""
    name, precision, (nx, ny), first, chunk, cap, eps = case
    assert oracle.precision == precision
    if case not in _runs:
        smp, nseg = ar.samples(oracle, name, nx, ny, cap)
        m2 = ar.welford_m2(smp, ar.rounds_of(first, chunk, cap))
        feat = features(oracle, name, nx, ny)
        rounds = schedule(lambda n_px: ar.expected_frame(smp, n_px), lambda k: ar.stderr_plane(m2[k], k), feat, nx, ny, first, chunk, cap, eps)
        _runs[case] = (smp, nseg, feat, rounds)
    return _runs[case]


# ---- hand-made maps for the retirement rule: (name, map, region, the tiles that must NOT retire although most of their pixels pass) -----------
def synthetic_maps(nx, ny, eps, region=None):
    """-> list of (what, noise [ny, nx], expected active [tiles_y, tiles_x] after one call on a frame whose local tiles are all active).
    The expectation is written per case from the rule, not computed by retire(): the CPU test compares the two."""
    tx, ty = fr.tiles_of(nx, ny)
    x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
    local = local_tiles(nx, ny, region)
    up = np.nextafter(eps, np.inf)
    out = []

    def case(what, fill, marks):
        """a map of `fill` with single pixels set: marks = [(x, y, value, keeps its tile?)]"""
        m = np.full((ny, nx), float(fill))
        active = np.zeros((ty, tx), bool) if fill <= eps else local.copy()
        for x, y, v, keeps in marks:
            m[y, x] = v
            inside = x0 <= x < x1 and y0 <= y < y1
            if keeps and inside:
                active[y // 8, x // 8] = True
        out.append((what, m, active & local))

    xl, yl = x1 - 1, y1 - 1  # the last pixel of the region: a partial tile at the right and bottom edge when the size is no multiple of 8
    case("exactly eps passes", eps, [])
    case("nextafter(eps, inf) fails", eps, [(x0, y0, up, True), (xl, yl, up, True), (xl, y0, up, True), (x0, yl, up, True)])
    case("everything fails", up, [])
    case("NaN and +inf fail, -inf and negative values pass", 0.0,
         [(x0 + 9, y0 + 1, np.nan, True), (x0 + 17, y0 + 9, np.inf, True), (x0 + 1, y0 + 9, -np.inf, False), (x0 + 2, y0 + 17, -1.0, False),
          (xl, yl, np.nan, True)])
    # one bad pixel per tile, walking through the 64 positions: every lane of the wave is looked at
    m = np.zeros((ny, nx))
    active = np.zeros((ty, tx), bool)
    n = 0
    for t_y in range(ty):
        for t_x in range(tx):
            if not local[t_y, t_x] or (t_y * tx + t_x) % 3 == 0:
                continue
            l = n % 64
            n += 1
            x, y = t_x * 8 + l % 8, t_y * 8 + l // 8
            if x < nx and y < ny:
                m[y, x] = np.inf
                active[t_y, t_x] = x0 <= x < x1 and y0 <= y < y1
    out.append(("one bad pixel per tile, every position", m, active))
    if region is not None:  # bad pixels outside the region, inside tiles the region cuts and in tiles it does not meet: not read
        m = np.full((ny, nx), np.nan)
        m[y0:y1, x0:x1] = eps
        out.append(("bad pixels outside the region are ignored", m, np.zeros((ty, tx), bool)))
    else:
        m = np.zeros((ny, nx))
        m[:, nx - 1] = np.inf  # the last column: the partial tiles at the right edge
        m[ny - 1, :] = np.inf  # the last row
        active = np.zeros((ty, tx), bool)
        active[:, tx - 1] = True
        active[ty - 1, :] = True
        out.append(("the last column and the last row", m, active))
    return out
