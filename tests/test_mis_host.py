"""Multiple importance sampling for the light-sampled paths, on the host: the restatements camera.mis_pick / mis_weight / mis_lobe / mis_closing against
a planar identity that tells the rule from its two wrong neighbours, the bound the rule exists for, the pick by power, and the MIS rule restated over
the CPU oracle's path logs (tests/mis_reference.py) against the oracle's plain paths -- the same expectation, with two negative controls that must fail
the same conditions.  No device is touched."""
import functools
import math

import numpy as np
import pytest

from raytrace_clj_amd import camera
from tests import direct_cases as dcs
from tests import direct_reference as dref
from tests import mis_cases as mcs
from tests import mis_reference as mref
from tests import nee_cases as ncs
from tests import nee_reference as nref


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


def _mean_se(a):
    return float(a.mean()), float(a.std(ddof=1) / math.sqrt(len(a)))


@pytest.mark.parametrize("h,rect", mcs.PLANAR)
def test_planar_identity(h, rect):
    """The shaded point at the origin, normal +z, an unoccluded rectangle of unit emission in the plane z = h, one light, the scatter n + b; 2^20 samples
    of each strategy.  light part + emission part = the hit fraction of an INDEPENDENT set of scatters within four combined standard errors (the three
    standard errors in quadrature), and every term is <= 1.  The controls are judged PAIRED -- the plain estimate taken from the same scatters as the
    emission part, so that the difference's standard error is that of the per-sample difference -- because unpaired the issue's own figures do not
    reach its bound at this count: in row 1 control B is off by 0.0021 and the plain estimate's standard error alone is 0.00023 at 2^20 samples (the
    issue's 13 standard errors are at 4 M).  Paired, control A (emission dropped) and control B (emission kept whole) each miss by more than ten
    standard errors, and the correct rule stays within four."""
    t = mcs.planar_terms(h, rect)
    (light, se_l), (emis, se_e), (plain, se_p) = _mean_se(t["light"]), _mean_se(t["emission"]), _mean_se(t["plain"])
    combined = math.sqrt(se_l ** 2 + se_e ** 2 + se_p ** 2)
    print("h %g: plain %.5f +- %.5f, nee %.5f +- %.5f (max %.1f), mis %.5f + %.5f = %.5f +- %.5f, largest term %.3f" % (
        h, plain, se_p, *_mean_se(t["nee"]), t["nee"].max(), light, emis, light + emis, math.sqrt(se_l ** 2 + se_e ** 2), max(t["light"].max(), t["emission"].max())))
    assert abs((light + emis) - plain) <= 4.0 * combined
    assert t["light"].max() <= 1.0 and t["emission"].max() <= 1.0 and t["light"].min() >= 0.0 and t["emission"].min() >= 0.0
    for name, diff, must_hold in (("mis", t["light"] + t["emission"] - t["whole"], True), ("control A", t["light"] - t["whole"], False),
                                  ("control B", t["light"], False)):  # (light + whole) - whole
        mean, se = _mean_se(diff)
        print("  paired %s: %.5f +- %.5f (%.1f standard errors)" % (name, mean, se, mean / se))
        assert (abs(mean) <= 4.0 * se) if must_hold else (abs(mean) > 10.0 * se), name


def _ceiling_point():
    """DESIGN.md section 7o's point: on the Cornell ceiling (y = 555, normal down), one unit from the lamp's edge, level with its middle"""
    f = dcs.flat("cornell")
    table = camera.light_table(f, dref.eligible(f))
    assert len(table) == 1 and table[0, 0] == 4.0  # one rect_xz lamp: x0, z0, x1, z1, y
    x0, z0, x1, z1, y = table[0, 1:6]
    return table, np.array([x0 - 1.0, y + 1.0, 0.5 * (z0 + z1)]), np.array([0.0, -1.0, 0.0])


def test_bounded_where_nee_is_not():
    n = 200000
    table, p, normal = _ceiling_point()
    rng = np.random.default_rng(5)
    ks, kp = rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    for choice in mcs.CHOICES:
        l, q, live = camera.mis_pick(table, kp, choice)
        _, d, w, built = camera.nee_samples(np.tile(p, (n, 1)), np.tile(normal, (n, 1)), table, ks, kp, light=l)
        x, m = camera.mis_weight(w, q[l])
        print("choice %d: largest w * nl %.1f, largest m %.6f, mean w %.4f, mean m %.4f" % (choice, (w * len(table)).max(), m.max(), w.mean(), m.mean()))
        assert built.any() and (w * len(table)).max() > 100.0 and m.max() <= 1.0 and m.min() >= 0.0
        assert np.array_equal(x, w * q[l]) and np.array_equal(m[built], (x / (1.0 + x))[built])


def test_every_contribution_of_a_log_is_bounded():
    """the rule restated over the oracle's Cornell paths (1 500 view rays, depth 3): add.c <= T.c * Le.c for every vertex of the log, exactly, and the
    closing weights lie in [0, 1], below 1 where the emission is weighted"""
    o, f = _oracle(), dcs.flat("cornell")
    lights = dref.eligible(f)
    rays, keys = dcs.view_rays(o, "cornell"), ncs.path_keys()
    table = camera.light_table(f, lights)
    for choice in mcs.CHOICES:
        rad, plain, s = mref.restate(o, f, rays, keys, 3, lights, choice, ctr0=2)
        cap = s["T"] * table[0, 7:10]
        assert (s["contrib"] <= cap).all() and s["contrib"].any() and (s["contrib"] >= 0.0).all()
        assert s["weighted"].any() and not s["weighted"].all() and (s["mq"] >= 0.0).all() and (s["mq"] <= 1.0).all() and (s["mq"][~s["weighted"]] == 1.0).all()
        assert (s["mq"][s["weighted"]] < 1.0).any() and (s["xq"][s["weighted"]] > 0.0).any()


def test_the_pick_by_power():
    n = 60000
    table = np.array([[3.0, 0.0, 0.0, 2.0, 1.0, 5.0, 2.0, 1.0, 2.0, 3.0],          # omega = 2 * 6 = 12
                      [0.0, 0.0, 9.0, 0.0, 1.0, 0.0, camera.FOURPI, 0.0, 0.0, 0.0],  # a lamp switched off: omega = 0
                      [4.0, 0.0, 0.0, 1.0, 4.0, 7.0, 4.0, 0.5, 0.25, 0.25]])        # omega = 4 * 1 = 4
    kp = np.random.default_rng(9).integers(0, 2 ** 63, n, dtype=np.uint64)
    l, q, live = camera.mis_pick(table, kp, 1)
    omega, W = np.array([12.0, 0.0, 4.0]), 16.0
    assert live.tolist() == [True, False, True] and not (l == 1).any()
    with np.errstate(divide="ignore"):
        assert np.array_equal(q, W / omega) and q[1] == np.inf
    for k in (0, 2):
        share = omega[k] / W
        assert abs((l == k).mean() - share) <= 4.0 * math.sqrt(share * (1.0 - share) / n), k
    # the dead light last: the fall-back index nl - 1 is never reached either
    l2, q2, live2 = camera.mis_pick(table[[0, 2, 1]], kp, 1)
    assert not (l2 == 2).any() and np.array_equal(l2 == 1, l == 2) and live2.tolist() == [True, True, False]
    # W = 0 (every lamp off), and a W that is not finite: the uniform pick with q = nl
    off = table.copy(); off[:, 7:10] = 0.0
    nan = table.copy(); nan[0, 7] = np.inf; nan[2, 7] = -np.inf
    uniform = camera.mis_pick(table, kp, 0)
    assert uniform[1].tolist() == [3.0, 3.0, 3.0] and uniform[2].all() and set(uniform[0].tolist()) == {0, 1, 2}
    for t in (off, nan):
        got = camera.mis_pick(t, kp, 1)
        assert all(np.array_equal(a, b) for a, b in zip(got, uniform))
    # one light: both choices pick it with q = 1
    one = camera.mis_pick(table[:1], kp, 1)
    assert not one[0].any() and one[1].tolist() == [1.0] and camera.mis_pick(table[:1], kp, 0)[1].tolist() == [1.0]
    with pytest.raises(ValueError):
        camera.mis_pick(table, kp, 2)


def test_lobe_and_closing_weight_edge_cases():
    g = camera.mis_lobe([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 0.0], [0, 0, 1.0], [np.nan, 0, 1.0]], [[0, 0, 3.0], [1.0, 0, 0], [0, 0, 1.0], [0, 0, 0.0], [0, 0, 1.0]])
    assert g.tolist() == [27.0 / 729.0, 0.0, 0.0, 0.0, 0.0]  # along the normal: 1 / |D|^3; edge-on, no normal, no direction, a NaN normal: +0.0
    assert camera.mis_lobe([[0, 0, 1.0]], [[0, 0, 1.0]], points=[[np.inf, 0, 0]]).tolist() == [0.0]
    x, m = camera.mis_closing([1.0, np.inf, np.nan, 0.0], np.tile([0, 0, 3.0], (4, 1)), np.tile([0, 0, -2.0], (4, 1)), [2.0] * 4, [4.0] * 4, [1.0] * 4)
    assert x[0] == (((1.0 * 2.0) / 4.0) * 4.0) * camera.TWO_INV_PI and m[0] == x[0] / (1.0 + x[0])
    assert x[1] == np.inf and m[1] == 1.0 and np.isnan(x[2]) and m[2] == 0.0 and m[3] == 0.0
    assert camera.mis_weight([np.inf, 0.0, 1.0], [2.0, 2.0, 3.0])[1].tolist() == [1.0, 0.0, 0.75]


@pytest.mark.parametrize("which", ("far", "near", "under"))
def test_same_estimand(which):
    """Scene sphere-lamp, depth 3, G = 48 groups of n = 4096 paths, the NEE tests' z-test (|mean z| <= 4 / sqrt(G), max |z| <= 5) against the oracle's plain
    paths, for both light choices.  far: nee_cases.estimand_inputs as it is; near: mis_cases.near_inputs at NEAR_SHARE; under: at UNDER_SHARE, the floor
    right under the lamp (the figures are in mis_cases' docstring).  The correct rule passes on all three; on the near sets control A (weighted
    emissions dropped) and control B (kept whole) fail at the same counts.  (They fail on the far set too, which only has to pass.)"""
    o = _oracle()
    f = dcs.flat(ncs.ESTIMAND_SCENE)
    lights = dref.eligible(f)
    rays, keys = ncs.estimand_inputs(o) if which == "far" else mcs.near_inputs(o, None if which == "near" else mcs.UNDER_SHARE)
    shape = (mcs.NEAR_G, mcs.NEAR_N, 3)
    for choice in mcs.CHOICES:
        mis, plain, s = mref.restate(o, f, rays, keys, ncs.ESTIMAND_DEPTH, lights, choice)
        z = nref.z_scores(plain.reshape(shape), mis.reshape(shape))
        print("%s, choice %d: mean z %.3f (bound %.3f), max |z| %.3f" % (which, choice, z.mean(), 4.0 / math.sqrt(len(z)), np.abs(z).max()))
        assert nref.same_estimand(z), z
        assert mis.reshape(shape).sum(axis=2).var(axis=1).mean() < 0.5 * plain.reshape(shape).sum(axis=2).var(axis=1).mean()
        if which == "far":
            continue
        for control in ("A", "B"):
            zc = nref.z_scores(plain.reshape(shape), mref.restate(o, f, rays, keys, ncs.ESTIMAND_DEPTH, lights, choice, control=control)[0].reshape(shape))
            print("  control %s: mean z %.3f, max |z| %.3f" % (control, zc.mean(), np.abs(zc).max()))
            assert not nref.same_estimand(zc), control


def test_choice_zero_restates_the_nee_rule_and_no_lights_is_the_plain_path():
    """with the uniform pick the light, its ray and w are the NEE rule's; an empty list is the plain path"""
    o, f = _oracle(), dcs.flat("example-light")
    lights = dref.eligible(f)
    rays, keys = dcs.view_rays(o, "example-light"), ncs.path_keys()
    rad, plain, s = mref.restate(o, f, rays, keys, 3, lights, 0, ctr0=2)
    rgb0, nseg, log, nlog = o.probe_paths(f, rays, keys, depth=3, ctr0=2, max_seg=4)
    i, j, l, d, w, built = nref.samples(log, nref.vertices(f, log, nlog), keys, camera.light_table(f, lights))
    assert np.array_equal(s["l"], l) and np.array_equal(mref.bits(s["d"]), mref.bits(d)) and np.array_equal(mref.bits(s["w"]), mref.bits(w))
    assert len(lights) == 2 and set(s["l"].tolist()) == {0, 1} and (s["q"] == 2.0).all()
    by_power = mref.restate(o, f, rays, keys, 3, lights, 1, ctr0=2)[2]
    assert not np.array_equal(by_power["l"], l) and not (by_power["q"] == 2.0).any()
    none, plain0, _ = mref.restate(o, f, rays, keys, 3, np.zeros(0, np.int32), ctr0=2)
    assert np.array_equal(mref.bits(none), mref.bits(plain0)) and not np.array_equal(mref.bits(rad), mref.bits(plain))


def test_mis_flag_parsing_and_refusals(monkeypatch):
    """--mis takes an optional word; what it does not combine with is refused before any device work (DeviceScene is never built)"""
    from raytrace_clj_amd import core

    def no_device(*a, **k):
        raise AssertionError("device work before the flags were checked")
    monkeypatch.setattr(core, "DeviceScene", no_device)
    monkeypatch.setattr(core, "render", no_device)
    assert core._mis_flags(["a.png", "--mis", "8"]) == (["a.png", "8"], "uniform")
    assert core._mis_flags(["a.png", "8", "--mis", "power"]) == (["a.png", "8"], "power")
    assert core._mis_flags(["--mis", "uniform", "a.png"]) == (["a.png"], "uniform")
    assert core._mis_flags(["a.png", "8", "--mis"]) == (["a.png", "8"], "uniform") and core._mis_flags(["a.png", "8"]) == (["a.png", "8"], None)
    assert core._mis_name("out/a.png") == "out/a.mis.png" and core.MIS_CHOICES == {"uniform": 0, "power": 1}
    for argv, word in ((["a.png", "8", "8", "1", "--mis=power"], "separate word"),
                       (["a.png", "8", "8", "1", "--mis", "--mis"], "twice"),
                       (["a.png", "8", "8", "1", "--mis", "--panorama"], "--panorama"),
                       (["a.png", "8", "8", "1", "--mis", "power", "--orbit", "4"], "--orbit"),
                       (["a.png", "8", "8", "1", "cornell-box", "--mis"], "ConstantMedium"),
                       (["a.png", "8", "8", "1", "subsurface-sphere", "--mis", "power"], "ConstantMedium")):
        with pytest.raises(SystemExit) as ei:
            core.main(argv)
        assert word in str(ei.value), (argv, ei.value)
    with pytest.raises(AssertionError):  # a scene it does trace gets as far as the device
        core.main(["a.png", "8", "8", "1", "cornell-box-classic", "--mis", "power"])
