"""Light-sampled paths on the host: camera.nee_samples against closed forms that tell the reference's scatter lobe 2 cos^3 / pi from the cosine lobe, and
the NEE rule restated over the CPU oracle's path logs (tests/nee_reference.py) against the oracle's plain paths -- the same expectation, with two
negative controls that must fail the same conditions.  No device is touched."""
import functools
import math

import numpy as np

from raytrace_clj_amd import camera
from tests import direct_cases as dcs
from tests import direct_reference as dref
from tests import nee_cases as ncs
from tests import nee_reference as nref


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(0, 2 ** 63, n, dtype=np.uint64)


def test_small_light_closed_form_tells_the_lobes_apart():
    """a 0.01 x 0.01 rectangle facing the point at distance 10, 60 degrees off the normal: every sample's w equals 2 cos^3 cos' A / (pi d^2), evaluated
    with the sample's own angles and distance through acos / cos, within 1e-5 -- half of what the cosine lobe gives.  (Across the light the value
    itself varies by 3 tan(60) x 5e-4 = 2.6e-3 relative, so it is each sample's own closed form that is compared, not the centre's.)"""
    n = 4096
    table = np.array([[3.0, -0.005, -0.005, 0.005, 0.005, 10.0, 1e-4, 1.0, 1.0, 1.0]])
    theta = math.radians(60.0)
    unit = np.array([math.sin(theta), 0.0, math.cos(theta)])
    ks, kp = _keys(n, 5)
    l, d, w, built = camera.nee_samples(np.zeros((n, 3)), np.tile(unit * 3.0, (n, 1)), table, ks, kp)  # (any length: the rule normalises)
    assert built.all() and (l == 0).all() and np.abs(d[:, :2]).max() <= 0.005 and (d[:, 2] == 10.0).all()
    dist = np.sqrt((d * d).sum(axis=1))
    theta_p, theta_l = np.arccos((d @ unit) / dist), np.arccos(d[:, 2] / dist)
    assert np.abs(np.degrees(theta_p) - 60.0).max() < 0.05
    want = 2.0 * np.cos(theta_p) ** 3 * np.cos(theta_l) * 1e-4 / (math.pi * dist ** 2)
    assert np.abs(w / want - 1.0).max() <= 1e-5
    cosine = np.cos(theta_p) * np.cos(theta_l) * 1e-4 / (math.pi * dist ** 2)
    assert np.abs(w / cosine - 0.5).max() <= 0.005  # 2 cos^2(60 degrees +- 0.03) = 0.5 +- 0.002: a factor of 2 apart


def test_inside_a_constant_dome_the_weights_average_one():
    """a point inside a sphere light sees the lobe's whole hemisphere: the mean of w over 2^16 samples is the lobe's integral, 1"""
    n = 1 << 16
    table = np.array([[0.0, 0.0, 0.0, 0.0, 10.0, 0.0, camera.FOURPI * 100.0, 1.0, 1.0, 1.0]])
    ks, kp = _keys(n, 6)
    l, d, w, built = camera.nee_samples(np.tile([3.0, -2.0, 1.0], (n, 1)), np.tile([0.2, 0.9, -0.4], (n, 1)), table, ks, kp)
    assert 0.3 < built.mean() < 0.7  # (the samples behind the point build no ray and weigh 0)
    se = w.std(ddof=1) / math.sqrt(n)
    assert abs(w.mean() - 1.0) <= 4.0 * se, (w.mean(), se)


def test_the_light_is_picked_uniformly_and_unbuilt_rows_are_zeros():
    n = 6000
    f = dcs.flat("example-light")
    table = camera.light_table(f, dref.eligible(f))
    assert len(table) == 2
    ks, kp = _keys(n, 7)
    rng = np.random.default_rng(8)
    l, d, w, built = camera.nee_samples(rng.normal(size=(n, 3)) * 3.0, rng.normal(size=(n, 3)), table, ks, kp)
    assert abs((l == 0).mean() - 0.5) < 0.03 and set(l.tolist()) == {0, 1}
    assert (~built).any() and not d[~built].any() and not w[~built].any() and (w[built] > 0.0).all()
    bad = np.zeros((2, 3)); bad[0, 0] = np.inf
    assert not camera.nee_samples(bad, np.ones((2, 3)) * [[1.0], [0.0]], table, ks[:2], kp[:2])[3].any()  # a non-finite point, a normal without length


def test_same_estimand():
    """Scene sphere-lamp, depth 3: G = 48 view rays whose first hit is Lambertian, each traced as n = 4096 paths; plain = the oracle, light-sampled = the
    restatement.  On the channel sum z_g = (m_nee - m_plain) / sqrt(v_nee / n + v_plain / n) must satisfy |mean z| <= 4 / sqrt(G) and max |z| <= 5.
    The two negative controls -- (a) step 6 off, (b) the cosine lobe -- each break a condition at these first counts (G = 48, n = 4096), which are
    therefore the counts the GPU test takes."""
    o = _oracle()
    f = dcs.flat(ncs.ESTIMAND_SCENE)
    lights = dref.eligible(f)
    rays, keys = ncs.estimand_inputs(o)
    shape = (ncs.ESTIMAND_G, ncs.ESTIMAND_N, 3)
    nee, plain = nref.restate(o, f, rays, keys, ncs.ESTIMAND_DEPTH, lights)
    z = nref.z_scores(plain.reshape(shape), nee.reshape(shape))
    print("z: mean %.3f (bound %.3f), max |z| %.3f" % (z.mean(), 4.0 / math.sqrt(len(z)), np.abs(z).max()))
    assert nref.same_estimand(z), z
    assert nee.reshape(shape).sum(axis=2).var(axis=1).mean() < 0.5 * plain.reshape(shape).sum(axis=2).var(axis=1).mean()  # and it is what the feature buys
    for control in ({"step6": False}, {"cosine": True}):
        zc = nref.z_scores(plain.reshape(shape), nref.restate(o, f, rays, keys, ncs.ESTIMAND_DEPTH, lights, **control)[0].reshape(shape))
        print("control %s: mean %.3f, max |z| %.3f" % (control, zc.mean(), np.abs(zc).max()))
        assert not nref.same_estimand(zc), control


def test_no_lights_is_the_plain_path():
    o = _oracle()
    f = dcs.flat("sphere-lamp")
    rays, keys = dcs.view_rays(o, "sphere-lamp"), ncs.path_keys()
    nee, plain = nref.restate(o, f, rays, keys, 3, np.zeros(0, np.int32), ctr0=2)
    assert np.array_equal(nref.bits(nee), nref.bits(plain)) and plain.any()
    some, _ = nref.restate(o, f, rays, keys, 3, dref.eligible(f), ctr0=2)
    assert not np.array_equal(nref.bits(some), nref.bits(plain))


def test_nee_flag_parsing_and_refusals(monkeypatch):
    """--nee is a switch; what it does not combine with is refused before any device work (DeviceScene is never built)"""
    import pytest

    from raytrace_clj_amd import core

    def no_device(*a, **k):
        raise AssertionError("device work before the flags were checked")
    monkeypatch.setattr(core, "DeviceScene", no_device)
    monkeypatch.setattr(core, "render", no_device)
    assert core._nee_flags(["a.png", "--nee", "8"]) == (["a.png", "8"], True)
    assert core._nee_flags(["a.png", "8"]) == (["a.png", "8"], False)
    assert core._nee_name("out/a.png") == "out/a.nee.png"
    for argv, word in ((["a.png", "8", "8", "1", "--nee=3"], "no value"),
                       (["a.png", "8", "8", "1", "--nee", "--panorama"], "--panorama"),
                       (["a.png", "8", "8", "1", "--nee", "--orbit", "4"], "--orbit"),
                       (["a.png", "8", "8", "1", "cornell-box", "--nee"], "ConstantMedium"),
                       (["a.png", "8", "8", "1", "subsurface-sphere", "--nee"], "ConstantMedium")):
        with pytest.raises(SystemExit) as ei:
            core.main(argv)
        assert word in str(ei.value), (argv, ei.value)
    with pytest.raises(AssertionError):  # a scene it does trace gets as far as the device
        core.main(["a.png", "8", "8", "1", "cornell-box-classic", "--nee"])
