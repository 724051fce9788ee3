"""Shared by test_reproject_reference.py (CPU), test_gpu_reproject.py (GPU) and scripts/eval_reproject.py: the numpy restatement of
rtmi_reproject, written from the text of include/rtmi.h alone -- vectorised over the pixels, the four taps in the stated order, every operation
one IEEE double operation as the header writes it -- the chain a TemporalAccumulator runs, and the analytic inputs of the tests (planes parallel
to the image plane of a pinhole camera, whose reprojection under a sideways move is a pure screen shift).
Nothing here imports the device library.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

import frame_reference as fr

FEATURES = 8
INF = float("inf")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def camera_parts(cam):
    """cam[24] -> origin, lleft, horiz, vert as tuples of three doubles (the only fields the operation reads)"""
    c = np.asarray(cam, np.float64)
    assert c.shape == (24,)
    return tuple(tuple(np.float64(x) for x in c[3 * k:3 * k + 3]) for k in range(4))


def reproject(nx, ny, prev_cam, cur_cam, prev_linear, prev_weight, prev_stderr, prev_features, cur_linear, cur_stderr, cur_features, cur_weight,
              max_history=INF, sigma_d=0.0, sigma_n=0.0, sigma_a=0.0):
    """rtmi_reproject restated -> (linear, rgb8, weight, stderr or None, counters uint64 [2], took bool [ny, nx]).  stderr is None unless both
    stderr inputs are given."""
    f8 = np.float64
    pl, pw, pf = np.asarray(prev_linear, f8), np.asarray(prev_weight, f8), np.asarray(prev_features, f8)
    cl, cf = np.asarray(cur_linear, f8), np.asarray(cur_features, f8)
    pse = None if prev_stderr is None else np.asarray(prev_stderr, f8)
    cse = None if cur_stderr is None else np.asarray(cur_stderr, f8)
    assert pl.shape == cl.shape == (ny, nx, 3) and pf.shape == cf.shape == (ny, nx, FEATURES) and pw.shape == (ny, nx)
    cw, mh = f8(cur_weight), f8(max_history)
    sd2, sn2, sa2 = f8(sigma_d) * f8(sigma_d), f8(sigma_n) * f8(sigma_n), f8(sigma_a) * f8(sigma_a)
    o, l, h, v = camera_parts(cur_cam)
    o1, l1, h1, v1 = camera_parts(prev_cam)
    with np.errstate(all="ignore"):
        # once per call
        a = tuple(l1[k] - o1[k] for k in range(3))
        n = _cross(h1, v1)
        nn = _dot(n, n)
        A = _dot(a, n)
        # 1. world point
        yy, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        jj = ny - 1 - yy
        uu = (ii.astype(f8) + 0.5) / f8(nx)
        vv = (jj.astype(f8) + 0.5) / f8(ny)
        d = tuple(((l[k] + uu * h[k]) + vv * v[k]) - o[k] for k in range(3))
        L = np.sqrt(_dot(d, d))
        s = cf[..., 6] / L
        P = tuple(o[k] + s * d[k] for k in range(3))
        # 2. into the previous camera
        q = tuple(P[k] - o1[k] for k in range(3))
        D = _dot(q, n)
        t = A / D
        ok = t > 0.0
        X = tuple(t * q[k] - a[k] for k in range(3))
        u1 = _dot(_cross(X, v1), n) / nn
        w1 = _dot(_cross(h1, X), n) / nn
        fx = u1 * f8(nx) - 0.5
        fy = f8(ny - 1) - (w1 * f8(ny) - 0.5)
        ok &= (fx > -1.0) & (fx < f8(nx)) & (fy > -1.0) & (fy < f8(ny))
        dist = np.sqrt(_dot(q, q))
        # 4. (first two conditions)
        ok &= (cf[..., 7] == 1.0) & np.isfinite(cl).all(axis=2)
        # 3. taps
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        W, N, T = np.zeros((ny, nx)), np.zeros((ny, nx)), np.zeros((ny, nx))
        S = [np.zeros((ny, nx)) for _ in range(3)]
        for ty in (0, 1):
            for tx in (0, 1):
                gx, gy = x0 + tx, y0 + ty
                acc = ok & (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny)
                gx, gy = np.clip(gx, 0, nx - 1), np.clip(gy, 0, ny - 1)
                b = (ax if tx else 1.0 - ax) * (ay if ty else 1.0 - ay)
                acc &= b > 0.0
                fq, wq, cq = pf[gy, gx], pw[gy, gx], pl[gy, gx]
                acc &= fq[..., 7] == 1.0
                acc &= np.isfinite(wq) & (wq > 0.0)
                acc &= np.isfinite(cq).all(axis=2)
                if pse is not None:
                    seq = pse[gy, gx]
                    acc &= ~np.isnan(seq)
                if sigma_d > 0:
                    dq = fq[..., 6]
                    e = dq - dist
                    m = np.where(dq > dist, dq, dist)
                    acc &= (e * e) <= sd2 * (m * m)
                if sigma_n > 0:
                    e = tuple(cf[..., 3 + k] - fq[..., 3 + k] for k in range(3))
                    acc &= _dot(e, e) <= sn2
                if sigma_a > 0:
                    e = tuple(cf[..., k] - fq[..., k] for k in range(3))
                    acc &= _dot(e, e) <= sa2
                W = np.where(acc, W + b, W)
                for ch in range(3):
                    S[ch] = np.where(acc, S[ch] + b * cq[..., ch], S[ch])
                N = np.where(acc, N + b * wq, N)
                if pse is not None:
                    T = np.where(acc, T + b * (seq * seq), T)
        # 4. blend
        took = W != 0.0
        Wd = np.where(took, W, 1.0)
        nh = N / Wd
        nh = np.where(nh > mh, mh, nh)
        w = nh + cw
        out = np.stack([np.where(took, (nh * (S[ch] / Wd) + cw * cl[..., ch]) / w, cl[..., ch]) for ch in range(3)], axis=2)
        weight = np.where(took, w, cw)
        stderr = None
        if pse is not None and cse is not None:
            V = ((nh * nh) * (T / Wd) + (cw * cw) * (cse * cse)) / (w * w)
            stderr = np.where(took, np.sqrt(V), cse)
    out = np.ascontiguousarray(out)
    return out, fr.quantise(out), weight, stderr, np.array([nx * ny, int(took.sum())], np.uint64), took


def accumulate(views, ns, max_history=INF, sigma_d=0.0, sigma_n=0.0, sigma_a=0.0):
    """the chain a TemporalAccumulator runs over `views` = [(cam24, linear, stderr, features), ...]: the first view starts without history (weight
    ns everywhere), every later one is reproject of the previous OUTPUT (linear, weight, stderr), the previous view's features and camera, and
    the current frame -> per view (linear, rgb8, weight, stderr, share of pixels with history)"""
    out, hist = [], None
    for cam, lin, se, ft in views:
        lin, se, ft = np.asarray(lin, np.float64), None if se is None else np.asarray(se, np.float64), np.asarray(ft, np.float64)
        ny, nx = lin.shape[:2]
        if hist is None:
            res = (lin.copy(), fr.quantise(lin), np.full((ny, nx), float(ns)), None if se is None else se.copy(), 0.0)
        else:
            o, q8, w, s, cnt, _ = reproject(nx, ny, hist[0], cam, hist[1], hist[2], hist[3], hist[4], lin, se, ft, float(ns), max_history, sigma_d,
                                            sigma_n, sigma_a)
            res = (o, q8, w, s, float(cnt[1]) / float(cnt[0]))
        out.append(res)
        hist = (np.asarray(cam, np.float64), res[0], res[2], res[3], ft)
    return out


# ---- analytic inputs: planes parallel to the image plane --------------------------------------------------------------------------------------------
def flat_camera(nx, ny, origin=(0.0, 0.0, 0.0), width=2.0, focus=1.0, kind=0):
    """a camera at `origin` looking down -z whose image plane at distance `focus` is `width` wide and width * ny / nx high: exact binary values for
    the sizes the tests use -> (kind, cam24); the lens fields hold values the operation must ignore"""
    ox, oy, oz = origin
    hw, hh = width / 2.0, width * ny / nx / 2.0
    cam = np.zeros(24)
    cam[0:3] = origin
    cam[3:6] = (ox - hw, oy - hh, oz - focus)
    cam[6:9] = (width, 0.0, 0.0)
    cam[9:12] = (0.0, 2.0 * hh, 0.0)
    cam[12:21] = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    cam[21:24] = (0.7, 0.25, 0.75) if kind else (0.0, 0.0, 0.0)
    return kind, cam


def pixel_rays(nx, ny, cam):
    """-> (origin [3], unit direction [ny, nx, 3]) of the pixel centres, row 0 = top (plain numpy: for building inputs, not part of the restatement)"""
    c = np.asarray(cam, np.float64)
    o, l, h, v = c[0:3], c[3:6], c[6:9], c[9:12]
    yy, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    u, w = (ii + 0.5) / nx, (ny - 1 - yy + 0.5) / ny
    d = l + u[..., None] * h + w[..., None] * v - o
    return o, d / np.linalg.norm(d, axis=2, keepdims=True)


def plane_view(nx, ny, cam, planes, colour):
    """what a camera sees of `planes` = [(z, x_lo, x_hi), ...] (each the part x_lo <= x <= x_hi of the plane at depth z < camera z, all facing +z):
    the nearest one hit per pixel centre -> (features [ny, nx, 8] with coverage 1 on a hit, colour(P) [ny, nx, 3], world points [ny, nx, 3],
    index of the plane hit or -1)"""
    o, d = pixel_rays(nx, ny, cam)
    best = np.full((ny, nx), np.inf)
    which = np.full((ny, nx), -1)
    for k, (z, x_lo, x_hi) in enumerate(planes):
        t = (z - o[2]) / d[..., 2]
        x = o[0] + t * d[..., 0]
        hit = (t > 0) & (x >= x_lo) & (x <= x_hi) & (t < best)
        best, which = np.where(hit, t, best), np.where(hit, k, which)
    hit = which >= 0
    t = np.where(hit, best, 0.0)
    P = o + t[..., None] * d
    ft = np.zeros((ny, nx, FEATURES))
    ft[..., 0:3] = np.where(hit[..., None], 0.25 + 0.125 * np.maximum(which, 0)[..., None], 0.0)
    ft[..., 5] = np.where(hit, 1.0, 0.0)
    ft[..., 6] = t
    ft[..., 7] = hit
    return ft, np.where(hit[..., None], colour(P), 0.0), P, which


def linear_colour(P):
    """a colour that is linear in world position: bilinear interpolation over pixels of a plane parallel to the image plane reproduces it exactly"""
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    return np.stack([0.5 + 0.25 * x + 0.125 * y, 0.75 - 0.125 * x + 0.0625 * z, 0.25 + 0.0625 * y - 0.03125 * z + 0.125 * x], axis=2)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
