"""CPU side of the volume rule (rtmi_render_rays_vol*, rtmi_probe_paths_vol, rtmi_render_lit_vol*): the entries exist and are declared, the argument
errors that stand before the handle check come back in the header's order, --lit-vol is parsed and refused before any device work, camera.vol_samples
and vol_lobe agree with nee_samples and with two closed forms of a lamp's solid angle, and the rule restated over the CPU oracle's parts
(tests/vol_reference.py) has the plain path tracer's expectation on the smoke box -- with two negative controls that must not.  No device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

from raytrace_clj_amd import _ffi, camera, core
from tests import direct_reference as dref
from tests import nee_reference as nref
from tests import vol_cases as vcs
from tests import vol_reference as vref

RTMI_E_ARG, RTMI_E_STATE = -1, -5
ENTRIES = (("rtmi_render_rays_vol", 19), ("rtmi_render_rays_vol_device", 20), ("rtmi_probe_paths_vol", 17), ("rtmi_render_lit_vol", 19),
           ("rtmi_render_lit_vol_device", 20))


# ---- 1. the entries and their first errors ------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_five_entries_and_ffi_declares_them():
    L = _ffi.lib()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name, n_args in ENTRIES:
        assert name in _ffi.SYMBOLS
        assert getattr(raw, name) is not None
        assert len(getattr(L, name).argtypes) == n_args
    assert _ffi.VOL_REC == vref.VOL_REC == _ffi.MIS_REC + 1 and core.VOL_ESTIMATORS == {"nee": 1, "mis": 2}


@pytest.mark.parametrize("device_form", [False, True])
def test_rays_argument_errors_in_the_headers_order(device_form):
    """with a NULL scene: rtmi_render_rays' own errors that precede the handle check, whatever the estimator, the lights and the choice, then RTMI_E_STATE"""
    L = _ffi.lib()
    rays, mean, se, cnt = np.zeros((8, 7)), np.full((8, 3), -7.0), np.full(8, -7.0), np.full(4, 9, np.uint64)
    err = lambda: L.rtmi_last_error().decode()

    def call(n_groups=8, group=1, g_first=0, depth=5, estimator=9, n_lights=-1, choice=5, precision=7, r=rays, m=mean, s=se):
        args = [None, precision, n_groups, group, g_first, core.ptr(r), None, 1, 0, depth, estimator, n_lights, None, choice, None, core.ptr(m), core.ptr(s),
                None, core.ptr(cnt)]
        return L.rtmi_render_rays_vol_device(*args, None) if device_form else L.rtmi_render_rays_vol(*args)
    for kw in (dict(n_groups=-1), dict(group=0), dict(g_first=-1), dict(depth=-1)):
        assert call(**kw) == RTMI_E_ARG and "n_groups" in err(), kw
    assert call(n_groups=1 << 16, group=1 << 16) == RTMI_E_ARG and "2^31 - 64" in err()
    assert call(g_first=(1 << 31) - 1) == RTMI_E_ARG and "overflows" in err()
    assert call(r=None) == RTMI_E_ARG and "rays" in err()
    assert call(m=None) == RTMI_E_ARG and call(s=None) == RTMI_E_ARG and "NULL" in err()
    for e in (-1, 0, 1, 2, 9):  # the handle comes before the precision, the estimator and the lights
        assert call(estimator=e) == RTMI_E_STATE and "scene" in err()
    assert (mean == -7.0).all() and (se == -7.0).all() and (cnt == 9).all()


@pytest.mark.parametrize("device_form", [False, True])
def test_lit_argument_errors_in_the_headers_order(device_form):
    """with a NULL scene: rtmi_render_lit's errors that precede the handle check -- its own estimator range 0..2 among them -- then RTMI_E_STATE: the
    volume rule's refusal of estimator 0 stands behind the list's length, which needs a scene"""
    L = _ffi.lib()
    lin, se = np.full((2, 2, 3), -7.0), np.full((2, 2), -7.0)
    err = lambda: L.rtmi_last_error().decode()

    def call(nx=2, ny=2, s_first=0, s_count=1, depth=5, estimator=2, out_linear=lin, out_stderr=se, n_lights=0, choice=0, precision=0):
        args = [None, precision, nx, ny, s_first, s_count, depth, 1, estimator, n_lights, None, choice, None, core.ptr(out_linear), None,
                core.ptr(out_stderr), None, None, None]
        return L.rtmi_render_lit_vol_device(*args, None) if device_form else L.rtmi_render_lit_vol(*args)
    bad = dict(estimator=9, out_linear=None, precision=7, n_lights=-1, choice=5)
    for kw in (dict(nx=0), dict(ny=0), dict(s_count=0), dict(s_first=-1), dict(depth=-1)):
        assert call(**dict(bad, **kw)) == RTMI_E_ARG and "s_count" in err(), kw
    assert call(**dict(bad, nx=1 << 16, ny=1 << 16)) == RTMI_E_ARG and "2^31 - 64" in err()
    assert call(**dict(bad, s_first=(1 << 31) - 1, s_count=1)) == RTMI_E_ARG and "overflows" in err()
    assert call(**bad) == RTMI_E_ARG and "NULL" in err()
    assert call(**dict(bad, out_linear=lin, out_stderr=None)) == RTMI_E_ARG and "NULL" in err()
    for e in (-1, 3, 9):
        assert call(**dict(bad, out_linear=lin, estimator=e)) == RTMI_E_ARG and "estimator" in err()
    for e in (0, 1, 2):
        assert call(**dict(bad, out_linear=lin, estimator=e)) == RTMI_E_STATE and "scene" in err()
    assert (lin == -7.0).all() and (se == -7.0).all()


def test_probe_argument_errors_in_the_headers_order():
    """rtmi_probe_paths' order: the handle first, whatever else is wrong; nothing is written"""
    L = _ffi.lib()
    rgb = np.full((4, 3), -7.0)
    for e in (-1, 0, 1, 2, 9):
        assert L.rtmi_probe_paths_vol(None, 7, -1, None, None, 0, 5, e, -1, None, 5, core.ptr(rgb), None, None, None, 0, None) == RTMI_E_STATE
    assert (rgb == -7.0).all()


def test_estimator_names_are_refused_before_any_device_work():
    ds = object.__new__(core.DeviceScene)  # no context, no handle: anything past the name check would fail on them
    for name in ("plain", "bdpt", "", "MIS"):
        with pytest.raises(ValueError):
            ds.render_lit_vol(8, 8, 1, estimator=name)
        with pytest.raises(ValueError):
            ds.render_rays_vol(np.zeros((1, 7)), estimator=name)
        with pytest.raises(ValueError):
            ds.probe_paths_vol(np.zeros((1, 7)), np.zeros(1, np.uint64), estimator=name)
    assert [core.DeviceScene._vol_estimator(n) for n in ("nee", "mis", 1, 2)] == [1, 2, 1, 2]


# ---- 2. the command line ------------------------------------------------------------------------------------------------------------------------------
def test_lit_vol_flag_parsing_and_refusals(monkeypatch):
    """--lit-vol takes an optional word; what it does not combine with is refused before any device work (DeviceScene is never built), and --lit on a
    media scene keeps its refusal and its message"""
    def no_device(*a, **k):
        raise AssertionError("device work before the flags were checked")
    monkeypatch.setattr(core, "DeviceScene", no_device)
    monkeypatch.setattr(core, "render", no_device)
    assert core._lit_vol_flags(["a.png", "--lit-vol", "8"]) == (["a.png", "8"], ("mis", "uniform"))
    assert core._lit_vol_flags(["a.png", "8", "--lit-vol"]) == (["a.png", "8"], ("mis", "uniform")) and core._lit_vol_flags(["a.png"]) == (["a.png"], None)
    assert core._lit_vol_flags(["a.png", "--lit-vol", "nee"]) == (["a.png"], ("nee", "uniform"))
    assert core._lit_vol_flags(["a.png", "--lit-vol", "mis:power", "8"]) == (["a.png", "8"], ("mis", "power"))
    assert core._lit_vol_flags(["a.png", "--lit-vol", "plain"]) == (["a.png", "plain"], ("mis", "uniform"))  # (no estimator of this flag: the next argument)
    assert core._lit_vol_name("out/a.png") == "out/a.vol.png"
    for argv, word in ((["a.png", "8", "8", "1", "--lit-vol=mis"], "separate word"),
                       (["a.png", "8", "8", "1", "--lit-vol", "--lit-vol"], "twice"),
                       (["a.png", "8", "8", "1", "--lit-vol", "nee:power"], "mis:power"),
                       (["a.png", "8", "8", "1", "--lit-vol", "mis:brightest"], "mis:power"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit-vol", "--panorama"], "--panorama"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit-vol", "mis:power", "--orbit", "4"], "--orbit"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit-vol", "--nee"], "--nee"),
                       (["a.png", "8", "8", "1", "cornell-box", "--mis", "power", "--lit-vol", "nee"], "--mis"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit-vol", "--lit", "plain"], "--lit"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit", "mis", "--lit-vol", "nee"], "--lit"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit"], "ConstantMedium"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit", "nee", "--chunk", "2"], "ConstantMedium")):
        with pytest.raises(SystemExit) as ei:
            core.main(argv)
        assert word in str(ei.value), (argv, ei.value)
    for argv in (["a.png", "8", "8", "1", "cornell-box", "--lit-vol", "mis:power", "--chunk", "2"], ["a.png", "8", "8", "1", "final", "--lit-vol", "nee"]):
        with pytest.raises(AssertionError):  # a combination it does render gets as far as the device
            core.main(argv)


# ---- 3. vol_samples and vol_lobe ----------------------------------------------------------------------------------------------------------------------
def _keys(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 63, n, dtype=np.uint64)


def _two_lamps():
    """a rect_xz lamp and a sphere lamp: rows of camera.light_table"""
    return np.array([[4.0, -1.0, -2.0, 3.0, 1.0, 5.0, 12.0, 1.0, 1.0, 1.0],
                     [0.0, 6.0, 1.0, -2.0, 1.5, 0.0, camera.FOURPI * (1.5 * 1.5), 2.0, 2.0, 2.0]])


def test_lambertian_rows_are_nee_samples_and_isotropic_rows_read_no_normal():
    n = 6000
    table = _two_lamps()
    ks, kp = _keys(n, 11)
    rng = np.random.default_rng(12)
    p, nrm = rng.normal(size=(n, 3)) * 3.0, rng.normal(size=(n, 3))
    iso = rng.random(n) < 0.5
    want = camera.nee_samples(p, nrm, table, ks, kp)
    got = camera.vol_samples(p, nrm, iso, table, ks, kp)
    lam = ~iso
    assert np.array_equal(got[0], want[0])  # the pick is one rule
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(vref.bits(a[lam]) if a.dtype != bool else a[lam], vref.bits(b[lam]) if b.dtype != bool else b[lam])
    none = camera.vol_samples(p, nrm, np.zeros(n, bool), table, ks, kp)
    assert all(np.array_equal(a, b) for a, b in zip(none, want))
    # an Isotropic row does not read its normal: any normal, a null one, a non-finite one give the same row; more rays are built than behind a surface
    for other in (-nrm, np.zeros((n, 3)), np.full((n, 3), np.nan)):
        again = camera.vol_samples(p, other, iso, table, ks, kp)
        assert all(np.array_equal(a[iso], b[iso]) for a, b in zip(again, got))
    assert got[3][iso].mean() > want[3][iso].mean() + 0.2 and (got[2][iso & got[3]] > 0.0).all()
    assert not got[1][~got[3]].any() and not got[2][~got[3]].any()
    bad = p.copy(); bad[iso, 0] = np.inf
    assert not camera.vol_samples(bad, nrm, iso, table, ks, kp)[3][iso].any()  # a point that is not finite builds no ray
    # the MIS rule's pick takes the pick's place
    forced = camera.vol_samples(p, nrm, iso, table, ks, kp, light=np.ones(n, np.int64))
    assert (forced[0] == 1).all()


def test_isotropic_weights_average_the_lamps_solid_angle():
    """the mean of w * q over many samples estimates (the lamp's solid angle) / 4 pi: a rectangle of half sides a, b seen from a point on its axis at
    height h, Omega = 4 atan(ab / (h sqrt(a^2 + b^2 + h^2))); a sphere of radius r at distance D, Omega = 2 pi (1 - sqrt(1 - r^2 / D^2)).  Tolerance:
    five standard errors of the sample mean."""
    n = 1 << 16
    iso = np.ones(n, bool)
    nrm = np.zeros((n, 3))
    a, b, h = 1.5, 1.0, 2.0
    rect = np.array([[4.0, -a, -b, a, b, h, 4.0 * a * b, 1.0, 1.0, 1.0]])
    ks, kp = _keys(n, 13)
    l, d, w, built = camera.vol_samples(np.zeros((n, 3)), nrm, iso, rect, ks, kp)
    assert built.all() and (d[:, 1] == h).all()
    want = 4.0 * math.atan(a * b / (h * math.sqrt(a * a + b * b + h * h))) / (4.0 * math.pi)
    se = w.std(ddof=1) / math.sqrt(n)
    print("rectangle: mean %.6f, closed form %.6f, standard error %.2g" % (w.mean(), want, se))
    assert abs(w.mean() - want) <= 5.0 * se and se < 0.01 * want
    r, D = 1.5, 4.0
    ball = np.array([[0.0, D, 0.0, 0.0, r, 0.0, camera.FOURPI * (r * r), 1.0, 1.0, 1.0]])
    ks, kp = _keys(n, 14)
    l, d, w, built = camera.vol_samples(np.zeros((n, 3)), nrm, iso, ball, ks, kp)
    assert 0.3 < built.mean() < 0.5  # (the far side builds no ray)
    want = 2.0 * math.pi * (1.0 - math.sqrt(1.0 - r * r / (D * D))) / (4.0 * math.pi)
    se = w.std(ddof=1) / math.sqrt(n)
    print("sphere: mean %.6f, closed form %.6f, standard error %.2g" % (w.mean(), want, se))
    assert abs(w.mean() - want) <= 5.0 * se and se < 0.02 * want
    # two lamps picked uniformly: w * q, q = 2, estimates each lamp's share in turn
    both = np.concatenate([rect, ball])
    ks, kp = _keys(n, 15)
    l, d, w, built = camera.vol_samples(np.zeros((n, 3)), nrm, iso, both, ks, kp)
    x, m = camera.mis_weight(w, np.full(n, 2.0))
    for k, omega in ((0, 4.0 * math.atan(a * b / (h * math.sqrt(a * a + b * b + h * h)))), (1, 2.0 * math.pi * (1.0 - math.sqrt(1.0 - r * r / (D * D))))):
        xs = np.where(l == k, x, 0.0)
        assert abs(xs.mean() - omega / (4.0 * math.pi)) <= 5.0 * xs.std(ddof=1) / math.sqrt(n)
    assert ((m >= 0.0) & (m < 1.0)).all()


def test_vol_lobe_times_the_closing_geometry_is_the_weight_at_the_point_the_scatter_found():
    """g * cl' / t^2 * area * TWO_INV_PI (what mis_closing forms) equals the step-3 weight at d = t * D, to a few ulps.  The bound: each side forms one
    three-term dot product of the lamp's normal with the direction, whose rounding error is at most 3 eps x the sum of the terms' magnitudes, that is
    3 eps / |cos| of its value -- the normals are drawn with |cos| >= 1/4, so 12 eps per side -- and some dozen other roundings of 1/2 ulp each: 40 eps."""
    n = 4096
    rng = np.random.default_rng(16)
    D = rng.normal(size=(n, 3)) * rng.uniform(0.2, 1.0, (n, 1))  # directions inside the unit ball, as the Isotropic scatter's
    t = rng.uniform(0.5, 30.0, n)
    unit = D / np.sqrt((D * D).sum(axis=1))[:, None]
    side = np.cross(unit, rng.normal(size=(n, 3))); side /= np.sqrt((side * side).sum(axis=1))[:, None]
    cos = rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)
    s = unit * cos[:, None] + side * np.sqrt(1.0 - cos * cos)[:, None]
    area = 7.0
    iso = np.ones(n, bool)
    g = camera.vol_lobe(np.zeros((n, 3)), D, iso, points=np.zeros((n, 3)))
    assert (g > 0.0).all()
    x, m = camera.mis_closing(g, s * 3.0, D, t, np.full(n, area), np.ones(n))
    d = D * t[:, None]
    d2 = (d * d).sum(axis=1)
    cl = np.abs((s * d).sum(axis=1))
    w = ((cl / (d2 * np.sqrt(d2))) * area) * camera.INV_4PI
    assert np.abs(x / w - 1.0).max() <= 40 * np.finfo(np.float64).eps
    assert 0.125 * camera.TWO_INV_PI == camera.INV_4PI  # the constant is exact
    # at a Lambertian vertex it is mis_lobe; a direction without length, or a point that is not finite, gives +0.0
    nrm = rng.normal(size=(n, 3))
    mixed = rng.random(n) < 0.5
    got = camera.vol_lobe(nrm, D, mixed)
    assert np.array_equal(vref.bits(got[~mixed]), vref.bits(camera.mis_lobe(nrm, D)[~mixed])) and np.array_equal(vref.bits(got[mixed]), vref.bits(g[mixed]))
    assert not camera.vol_lobe(nrm, np.zeros((n, 3)), iso).any()
    assert not camera.vol_lobe(nrm, D, iso, points=np.full((n, 3), np.inf)).any()


# ---- 4. the same estimand, on the oracle ----------------------------------------------------------------------------------------------------------------
def test_the_groups_are_what_the_geometry_says(oracle):
    assert vcs.media_lie_below_the_lamp()
    f = vcs.flat("smoke")
    lights = dref.eligible(f)
    table = camera.light_table(f, lights)
    assert len(table) == 1 and table[0, 0] == 4.0 and tuple(table[0, 1:6]) == vcs.LAMP  # the one lamp, where the recipes say it is
    rays, keys, kind = vcs.estimand_inputs(oracle)
    assert (kind == 0).sum() == (kind == 1).sum() == vcs.ESTIMAND_G // 2
    # the first vertex of most paths of a smoke group is an Isotropic scatter in the white smoke; no first vertex of a floor group is
    n = 64
    pick = (np.arange(vcs.ESTIMAND_G)[:, None] * vcs.ESTIMAND_N + np.arange(n)[None, :]).ravel()
    _, nseg, log, nlog = oracle.probe_paths(f, rays[pick], keys[pick], depth=1, ctr0=0, max_seg=2)
    at, iso = vref.vertices(f, log, nlog)
    first_iso = iso[:, 0].reshape(vcs.ESTIMAND_G, n).mean(axis=1)
    white = np.asarray(f.tex_param, np.float64).reshape(-1, 12)[np.asarray(f.mat_tex)[np.asarray(f.prim_mat)[log[iso[:, 0], 0, 0].astype(np.int64)]], 0:3]
    assert (first_iso[kind == 0] > 0.6).all() and (first_iso[kind == 1] == 0.0).all() and (white == 1.0).all()
    assert (np.abs(log[:, 0, 3].reshape(vcs.ESTIMAND_G, n)[kind == 1]) < 1e-9).all() and at[:, 0].reshape(vcs.ESTIMAND_G, n)[kind == 1].all()


@pytest.mark.parametrize("estimator, choice", vcs.ESTIMATORS[:2])
def test_same_estimand(oracle, estimator, choice):
    """The smoke box, depth 3: G = 48 groups of n = 4096 paths (nee_cases' sizes), half of them first vertices in the white smoke, half floor points
    whose segment to the lamp crosses a smoke block; plain = the oracle, light-sampled = the restated chain over the oracle's parts.  On the channel
    sum z_g must satisfy |mean z| <= 4 / sqrt(G) and max |z| <= 5 (nee_reference.same_estimand).  Two negative controls must fail the same condition:
    shadow flags from the box without its media on the floor groups, and the closing emission kept whole behind an Isotropic light sample on the
    smoke groups."""
    f = vcs.flat("smoke")
    lights = dref.eligible(f)
    rays, keys, kind = vcs.estimand_inputs(oracle)
    G, n = vcs.ESTIMAND_G, vcs.ESTIMAND_N
    vol, plain, s = vref.restate(oracle, f, rays, keys, vcs.ESTIMAND_DEPTH, lights, estimator, choice)
    z = nref.z_scores(plain.reshape(G, n, 3), vol.reshape(G, n, 3))
    print("estimator %d: z mean %.3f (bound %.3f), max |z| %.3f" % (estimator, z.mean(), 4.0 / math.sqrt(G), np.abs(z).max()))
    assert nref.same_estimand(z), z
    assert s["iso"].any() and (~s["iso"]).any() and s["occluded"][s["iso"]].any() and s["free"][s["iso"]].any()
    floor, smoke = np.repeat(kind == 1, n), np.repeat(kind == 0, n)
    clear, _, _ = vref.restate(oracle, f, rays[floor], keys[floor], vcs.ESTIMAND_DEPTH, lights, estimator, choice, shadow_flat=vcs.clear_flat())
    zc = nref.z_scores(plain[floor].reshape(-1, n, 3), clear.reshape(-1, n, 3))
    print("control, media ignored by shadow rays: mean %.3f, max |z| %.3f" % (zc.mean(), np.abs(zc).max()))
    assert not nref.same_estimand(zc)
    twice, _, _ = vref.restate(oracle, f, rays[smoke], keys[smoke], vcs.ESTIMAND_DEPTH, lights, estimator, choice, keep_after_iso=True)
    zd = nref.z_scores(plain[smoke].reshape(-1, n, 3), twice.reshape(-1, n, 3))
    print("control, closing emission kept behind an Isotropic sample: mean %.3f, max |z| %.3f" % (zd.mean(), np.abs(zd).max()))
    assert not nref.same_estimand(zd)
