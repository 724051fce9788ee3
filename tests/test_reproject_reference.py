"""CPU tests of the numpy restatement of rtmi_reproject (tests/reproject_reference.py), against expectations that do not come from it:

  * an analytic case: a plane parallel to the image plane, a colour linear in world position, the camera moved sideways by 2.25 pixels -- bilinear
    interpolation is then exact and the reprojected history must be the colour at the current pixel's world point;
  * disocclusion: two such planes shift by different amounts, and the band of the far plane that the near one hid takes no history;
  * the identity camera: the plain weighted mean, the weights add, the standard error follows its formula;
  * every rejection on its own;
  * on the oracle's Cornell box the accumulated frame is closer to the truth than the raw one, and not vacuously.

Tolerances: the analytic values are compared to 1e-12: coordinates here are O(1), one reprojection is a few dozen double
operations, so the error is a few hundred ulps of 1, i.e. below 1e-13."""
import numpy as np
import pytest

import frame_reference as fr
import reproject_reference as rr

NX, NY = 64, 32      # pixel width 2 / 64 on the image plane at distance 1: exact binary values
Z = -4.0             # the plane: its pixel footprint is 4 * 2 / 64 = 0.125 world units
SHIFT = 2.25         # pixels


def _frames(planes_prev, planes_cur=None, dx=SHIFT * 0.125, kind=0, nx=NX, ny=NY):
    """history seen from the origin, current frame from a camera moved by dx along +x: a plane at depth 4 then moves by -dx / 0.125 pixels"""
    _, cam0 = rr.flat_camera(nx, ny, kind=kind)
    _, cam1 = rr.flat_camera(nx, ny, origin=(dx, 0.0, 0.0), kind=kind)
    ft0, col0, _, _ = rr.plane_view(nx, ny, cam0, planes_prev, rr.linear_colour)
    ft1, col1, P1, which1 = rr.plane_view(nx, ny, cam1, planes_cur or planes_prev, rr.linear_colour)
    return cam0, cam1, ft0, col0, ft1, col1, P1, which1


WIDE = [(Z, -100.0, 100.0)]


def test_sideways_move_is_an_exact_screen_shift():
    cam0, cam1, ft0, col0, ft1, col1, P1, _ = _frames(WIDE)
    w0 = np.full((NY, NX), 8.0)
    cur = np.zeros((NY, NX, 3))  # a current frame of zeros with weight 1: out = n_h c_h / (n_h + 1), so c_h can be read back
    out, q8, w, se, cnt, took = rr.reproject(NX, NY, cam0, cam1, col0, w0, None, ft0, cur, None, ft1, 1.0)
    assert se is None
    # the history of current pixel i lies at previous column i + 2.25: taps i + 2 and i + 3 must be inside the image
    cols = np.arange(NX)
    inside = np.broadcast_to(cols + 3 <= NX - 1, (NY, NX))
    assert took[inside].all() and inside.sum() == NY * (NX - 3)
    assert np.array_equal(w[inside], np.full(inside.sum(), 9.0))
    c_h = out * 9.0 / 8.0
    err = np.abs(c_h - rr.linear_colour(P1))[inside].max()
    print("largest error of the reprojected history on the analytic plane: %.3g" % err)
    assert err <= 1e-12
    # column NX - 3 has its right-hand taps at NX - 1 + ... : one column of taps outside -> still history from the taps inside, renormalised
    assert took[:, NX - 3].all() and not took[:, NX - 2:].any(), "2.25 pixels: the last two columns project outside (-1 < fx < nx fails at 64.25, 65.25)"
    assert int(cnt[0]) == NX * NY and int(cnt[1]) == took.sum()
    assert np.array_equal(out[~took], cur[~took]) and np.array_equal(w[~took], np.ones((~took).sum()))
    assert np.array_equal(q8, fr.quantise(out))


def test_thin_lens_is_reprojected_through_its_centre():
    a = _frames(WIDE, kind=0)
    b = _frames(WIDE, kind=1)
    w0 = np.full((NY, NX), 3.0)
    ra = rr.reproject(NX, NY, a[0], a[1], a[3], w0, None, a[2], a[5], None, a[4], 2.0, sigma_d=0.05, sigma_n=0.5, sigma_a=0.5)
    rb = rr.reproject(NX, NY, b[0], b[1], b[3], w0, None, b[2], b[5], None, b[4], 2.0, sigma_d=0.05, sigma_n=0.5, sigma_a=0.5)
    assert not np.array_equal(a[0], b[0]), "the lens fields differ"
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2]) and ra[5].sum() > 0


def test_disocclusion_band_takes_no_history():
    """a near plane at depth 2 covering x <= 0 in front of the far plane at depth 4: the camera moves by dx = 0.5625, the near plane shifts by
    dx / (2 * 2 / 64) = 9 pixels, the far plane by 4.5: the far-plane pixels uncovered by the move have both their taps on the near plane"""
    dx = 0.5625
    planes = [(-2.0, -100.0, 0.0), (Z, -100.0, 100.0)]
    cam0, cam1, ft0, col0, ft1, col1, P1, which1 = _frames(planes, dx=dx)
    w0 = np.full((NY, NX), 8.0)
    out, _, w, _, cnt, took = rr.reproject(NX, NY, cam0, cam1, col0, w0, None, ft0, np.zeros((NY, NX, 3)), None, ft1, 1.0, sigma_d=0.05)
    # analytic: the near plane's edge x = 0 is seen at image-plane x = (0 - camera x) / 2, i.e. at the pixel boundary (that + 1) * 32
    edge_prev = int((0.0 - 0.0) / 2.0 * 32 + 32)   # 32: columns < 32 show the near plane in the previous frame
    edge_cur = int((0.0 - dx) / 2.0 * 32 + 32)     # 23: columns < 23 show it now
    assert (edge_prev, edge_cur) == (32, 23)
    assert (which1[:, :edge_cur] == 0).all() and (which1[:, edge_cur:] == 1).all()
    # far-plane pixel i has its history at column i + 4.5, taps i + 4 and i + 5: both showed the near plane while i + 5 <= 31
    band_end = edge_prev - 5
    band = np.zeros((NY, NX), bool)
    band[:, edge_cur:band_end] = True
    assert band_end - edge_cur == 4
    assert not took[band].any(), "the uncovered band takes no history"
    width = (~took[:, edge_cur:NX - 5]).sum(axis=1)
    assert (width == band_end - edge_cur).all(), width
    near_ok = np.zeros((NY, NX), bool)
    near_ok[:, :edge_cur] = True                # near plane: history at i + 9 <= 31, still the near plane
    far_ok = np.zeros((NY, NX), bool)
    far_ok[:, edge_prev - 4:NX - 5] = True      # far plane with both taps on the far plane and inside the image
    assert took[near_ok].all() and took[far_ok].all() and took[:, band_end].all()
    c_h = out * 9.0 / 8.0
    assert np.abs(c_h - rr.linear_colour(P1))[near_ok | far_ok].max() <= 1e-12
    # without the depth test the band would have taken the near plane's colour: the test is what rejects it
    took_off = rr.reproject(NX, NY, cam0, cam1, col0, w0, None, ft0, np.zeros((NY, NX, 3)), None, ft1, 1.0)[5]
    assert took_off[band].all()


def _identity_inputs(nx=23, ny=17, seed=3):
    rng = np.random.default_rng(seed)
    _, cam = rr.flat_camera(nx, ny)
    ft, _, _, _ = rr.plane_view(nx, ny, cam, [(Z, -0.5, 100.0)], rr.linear_colour)  # the left part of the view misses: coverage 0 there
    cp, cc = rng.random((ny, nx, 3)), rng.random((ny, nx, 3))
    wp = rng.integers(1, 40, (ny, nx)).astype(np.float64)
    sp, sc = 0.1 * rng.random((ny, nx)), 0.2 * rng.random((ny, nx))
    return nx, ny, cam, ft, cp, cc, wp, sp, sc


def test_identity_camera_is_the_weighted_mean():
    nx, ny, cam, ft, cp, cc, wp, sp, sc = _identity_inputs()
    wc = 4.0
    out, q8, w, se, cnt, took = rr.reproject(nx, ny, cam, cam, cp, wp, sp, ft, cc, sc, ft, wc, sigma_d=0.05, sigma_n=0.5, sigma_a=0.2)
    cov = ft[..., 7] == 1.0
    assert 0 < cov.sum() < nx * ny
    assert np.array_equal(took, cov) and int(cnt[1]) == cov.sum()
    want = (wp[..., None] * cp + wc * cc) / (wp[..., None] + wc)
    assert np.abs(out - want)[cov].max() <= 1e-12
    assert np.abs(w - (wp + wc))[cov].max() <= 1e-12
    want_se = np.sqrt((wp * wp * sp * sp + wc * wc * sc * sc) / ((wp + wc) ** 2))
    assert np.abs(se - want_se)[cov].max() <= 1e-12
    # no history: colour and stderr bit for bit, the weight is the current frame's
    assert np.array_equal(out[~cov], cc[~cov]) and np.array_equal(se[~cov], sc[~cov]) and (w[~cov] == wc).all()
    # the cap
    capped = rr.reproject(nx, ny, cam, cam, cp, wp, sp, ft, cc, sc, ft, wc, max_history=10.0)
    nh = np.minimum(wp, 10.0)
    assert np.abs(capped[2] - (nh + wc))[cov].max() <= 1e-12 and (wp > 10).any() and (wp < 10).any()
    assert np.abs(capped[0] - (nh[..., None] * cp + wc * cc) / (nh[..., None] + wc))[cov].max() <= 1e-12
    assert np.abs(capped[3] - np.sqrt((nh * nh * sp * sp + wc * wc * sc * sc) / ((nh + wc) ** 2)))[cov].max() <= 1e-12


def test_every_rejection_on_its_own():
    nx, ny, cam, ft, cp, cc, wp, sp, sc = _identity_inputs()
    run = lambda **kw: rr.reproject(nx, ny, kw.pop("prev_cam", cam), kw.pop("cur_cam", cam), kw.pop("cp", cp), kw.pop("wp", wp), kw.pop("sp", sp),
                                    kw.pop("fp", ft), kw.pop("cc", cc), kw.pop("sc", sc), kw.pop("fc", ft), 4.0, **kw)
    # the pixel under test, well inside the covered part; the history's coverage is 0 on the ring around it: with the identity camera fx and fy
    # are whole numbers up to rounding, and a neighbouring tap of weight 1e-16 must not stand in for the rejected one
    y, x = ny // 2, nx - 4
    ring = np.zeros((ny, nx), bool)
    ring[y - 1:y + 2, x - 1:x + 2] = True
    ring[y, x] = False
    ft_prev = ft.copy()
    ft_prev[ring, 7] = 0.0
    run0 = run
    run = lambda **kw: run0(**dict(dict(fp=ft_prev), **kw))
    base = run()[5]
    assert base[y, x] and (ft[y - 1:y + 2, x - 1:x + 2, 7] == 1.0).all()

    def poisoned(a, value, ch=None):
        b = a.copy()
        if ch is None:
            b[y, x] = value
        else:
            b[y, x, ch] = value
        return b

    def only_that_pixel(took):
        d = took != base
        elsewhere = ~ring
        elsewhere[y, x] = False
        return bool(d[y, x]) and not d[elsewhere].any()

    def unchanged(took):  # (the ring's own pixels live on taps of weight 1e-16 or on none: they are not judged)
        d = took != base
        elsewhere = ~ring
        return not d[elsewhere].any()

    for value in (np.nan, np.inf, -np.inf):
        for ch in range(3):
            assert only_that_pixel(run(cp=poisoned(cp, value, ch))[5]), ("history colour", value, ch)
            r = run(cc=poisoned(cc, value, ch))
            assert only_that_pixel(r[5]) and np.array_equal(r[0][y, x], poisoned(cc, value, ch)[y, x], equal_nan=True), ("own colour", value, ch)
    for value in (0.0, -1.0, np.nan, np.inf):
        assert only_that_pixel(run(wp=poisoned(wp, value))[5]), ("weight", value)
    assert only_that_pixel(run(fp=poisoned(ft_prev, 0.5, 7))[5]) and only_that_pixel(run(fc=poisoned(ft, 0.5, 7))[5]), "coverage 0.5, either side"
    assert only_that_pixel(run(sp=poisoned(sp, np.nan))[5]), "NaN history stderr"
    r = run(sp=poisoned(sp, np.inf))
    assert np.array_equal(r[5], base) and r[3][y, x] == np.inf and np.isfinite(r[0][y, x]).all(), "+inf history stderr is taken and gives +inf"
    r = run(sc=poisoned(sc, np.inf))
    assert np.array_equal(r[5], base) and r[3][y, x] == np.inf
    r = run(sp=None)
    assert r[3] is None and np.array_equal(r[5], base) and np.array_equal(r[0], run()[0]), "absent stderr changes nothing else"
    assert run(sc=None)[3] is None
    # a camera turned by 180 degrees: the world points lie behind it (t <= 0)
    back = cam.copy()
    back[3:6] = (1.0, cam[4], 1.0)
    back[6:9] = (-2.0, 0.0, 0.0)
    assert not run(prev_cam=back)[5].any() and not run(cur_cam=back)[5].any()
    # a target outside the frame: the previous camera far to the side
    _, far = rr.flat_camera(nx, ny, origin=(40.0, 0.0, 0.0))
    assert not run(prev_cam=far)[5].any()
    # each sigma, just inside and just outside its threshold, and off
    for ch, name, delta in ((6, "sigma_d", None), (3, "sigma_n", 0.25), (0, "sigma_a", 0.25)):
        if delta is None:   # depth: e = dq - dist against sigma * max(dq, dist): dq = dist * 1.25 -> e / m = 0.2 (in exact arithmetic)
            fp = poisoned(ft_prev, ft[y, x, 6] * 1.25, 6)
            lo, hi = 0.2 * (1 - 1e-9), 0.2 * (1 + 1e-9)
        else:
            fp = poisoned(ft_prev, ft[y, x, ch] + delta, ch)
            lo, hi = delta * (1 - 1e-9), delta * (1 + 1e-9)
        assert only_that_pixel(run(fp=fp, **{name: lo})[5]), (name, "just outside")
        assert unchanged(run(fp=fp, **{name: hi})[5]), (name, "just inside")
        assert unchanged(run(fp=fp, **{name: 0.0})[5]), (name, "off")
        others = {n: 1e-3 for n in ("sigma_d", "sigma_n", "sigma_a") if n != name}
        assert unchanged(run(fp=fp, **others)[5]), (name, "the other tests do not read this channel")


# ---- it helps: the oracle's Cornell box ---------------------------------------------------------------------------------------------------------------
def cornell_views(oracle, nx, ny, views, degrees, ns, na=4, truth_spp=256):
    """`views` pinhole views of the classic Cornell box turned about the vertical axis through its centre, each rendered by the oracle with ns
    samples and its own seed, with features from the probes -> ([(cam24, linear, stderr, features)], truth of the last view)"""
    import raytrace_clj_amd as r
    import denoise_reference as dr
    from oracle.tree import attach_tree
    from raytrace_clj_amd import flatten as fl
    from raytrace_clj_amd.util import vec3
    world = r.scene.make_cornell_box(nx, ny)["world"]
    out, flat = [], None
    for k in range(views):
        a = np.radians(degrees * k)
        frm = vec3(278 + 1078 * np.sin(a), 278, 278 - 1078 * np.cos(a))
        cam = r.camera.pinhole_camera(lookfrom=frm, lookat=vec3(278, 278, 278), vup=vec3(0, 1, 0), vfov=40, aspect=nx / ny)
        flat = attach_tree(fl.flatten({"camera": cam, "world": world}), world)
        smp, _ = fr.frame_samples(oracle, flat, nx, ny, ns, seed=fr.SEED + k)
        lin = fr.frame_in_order(smp)
        se = fr.stderr_two_pass(smp, ns)
        ft = dr.feature_frame(dr.feature_samples(oracle, flat, nx, ny, na, seed=fr.SEED + k))
        out.append((np.asarray(flat.cam, np.float64), lin, se, ft))
    truth = oracle.render(flat, nx, ny, truth_spp, fr.DEPTH, fr.SEED + 1000, nthreads=16)[0]
    return out, truth


def test_accumulation_helps_on_the_cornell_box(oracle):
    nx = ny = 96
    views, truth = cornell_views(oracle, nx, ny, 6, 1.0, 4)
    from raytrace_clj_amd import core
    res = rr.accumulate(views, 4, core.REPROJECT_MAX_HISTORY, core.REPROJECT_SIGMA_D, core.REPROJECT_SIGMA_N, core.REPROJECT_SIGMA_A)
    raw, acc, share = rr.rms(views[-1][1], truth), rr.rms(res[-1][0], truth), res[-1][4]
    print("cornell 96x96, 6 views 1 degree apart, 4 spp: rms raw %.4f accumulated %.4f ratio %.3f, history on %.3f of the pixels, mean weight %.2f"
          % (raw, acc, acc / raw, share, res[-1][2].mean()))
    assert acc / raw < 1.0
    assert share >= 0.75
