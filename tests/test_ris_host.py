"""The proposal rule for the light-sampled paths, on the host: the header's constants and symbols, the error order through the host-only paths, the flag
parsing, the restatements camera.ris_candidates / ris_choose against a planar identity that tells the rule from its two wrong neighbours, the rule's bound,
the variance statement against the MIS rule under both picks, and the near set of the device's expectation test -- all over the CPU oracle's path logs
(tests/ris_reference.py).  No device is touched."""
import functools
import math
import os
import re

import numpy as np
import pytest

from raytrace_clj_amd import _ffi, camera, core, util
from tests import direct_reference as dref
from tests import mis_cases as mcs
from tests import mis_reference as mref
from tests import nee_cases as ncs
from tests import nee_reference as nref
from tests import ris_cases as rcs
from tests import ris_reference as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rtmi_render_rays_ris", "rtmi_render_rays_ris_device", "rtmi_probe_paths_ris", "rtmi_render_lit_ris", "rtmi_render_lit_ris_device")


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("f64")


def _mean_se(a):
    return float(a.mean()), float(a.std(ddof=1) / math.sqrt(len(a)))


def test_header_constants_and_symbols():
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert int(re.search(r"#define RTMI_RIS_REC (\d+)", header).group(1)) == _ffi.RIS_REC == rref.RIS_REC == _ffi.MIS_REC + 4 == 32
    assert "THE PROPOSAL RULE" in header
    for name in NEW:
        assert name in _ffi.SYMBOLS and re.search(r"\bint %s\(" % name, header), name
    L = _ffi.lib()  # binds every symbol: a missing kernel entry is an error, not a fall-back
    assert len(L.rtmi_render_lit_ris.argtypes) == len(L.rtmi_render_lit_tiles.argtypes) - 3
    assert len(L.rtmi_render_lit_ris_device.argtypes) == len(L.rtmi_render_lit_tiles_device.argtypes) - 3
    assert len(L.rtmi_render_rays_ris.argtypes) == len(L.rtmi_render_rays_mis.argtypes) - 1
    assert len(L.rtmi_probe_paths_ris.argtypes) == len(L.rtmi_probe_paths_mis.argtypes) - 1


def test_error_order_through_the_host_only_paths():
    """the argument checks that stand in front of the scene handle need no device: a NULL handle is reported (RTMI_E_STATE) only behind them"""
    L = _ffi.lib()
    buf = np.zeros(64)
    p = core.ptr(buf)
    tiles = np.zeros(4, np.int32)

    def frame(nx=8, ny=8, s_first=0, s_count=1, depth=1, n_tiles=0, t=None, lin=p, se=p):
        return L.rtmi_render_lit_ris(None, 0, nx, ny, s_first, s_count, depth, 1, 0, None, n_tiles, core.ptr(t), None, lin, None, se, None, None, None)
    assert frame(nx=0) == -1 and frame(ny=-1) == -1 and frame(s_count=0) == -1 and frame(s_first=-1) == -1 and frame(depth=-1) == -1
    assert frame(nx=1 << 16, ny=1 << 16) == -1 and frame(s_first=2 ** 31 - 1, s_count=1) == -1
    assert frame(lin=None) == -1 and frame(se=None) == -1
    assert frame(n_tiles=-1, t=tiles) == -1 and frame(n_tiles=2, t=np.array([0, 7], np.int32)) == -1          # an entry outside the frame's one tile
    assert frame(nx=16, n_tiles=2, t=np.array([1, 0], np.int32)) == -1 and b"ascending" in L.rtmi_last_error()
    assert frame() == -5 and frame(n_tiles=1, t=tiles) == -5 and frame(n_tiles=-1) == -5                        # tiles NULL: n_tiles is not read
    # the rays call: rtmi_render_rays' own checks first, whatever the lights are
    many = np.zeros(_ffi.DIRECT_MAX_LIGHTS + 1, np.int32)

    def rays(n_groups=1, group=1, g_first=0, depth=1, r=p, m=p):
        return L.rtmi_render_rays_ris(None, 0, n_groups, group, g_first, r, None, 1, 0, depth, len(many), core.ptr(many), None, m, p, None, None)
    assert rays(n_groups=-1) == -1 and rays(group=0) == -1 and rays(g_first=-1) == -1 and rays(depth=-1) == -1 and rays(r=None) == -1 and rays(m=None) == -1
    assert rays() == -5


def test_flag_parsing(monkeypatch):
    """--lit ris is a word of --lit; what --lit does not combine with is refused before any device work (DeviceScene is never built)"""
    def no_device(*a, **k):
        raise AssertionError("device work before the flags were checked")
    refine = core.DeviceScene.refine_lit_adaptive
    monkeypatch.setattr(core, "DeviceScene", no_device)
    monkeypatch.setattr(core, "render", no_device)
    assert core._lit_flags(["a.png", "--lit", "ris", "8"]) == (["a.png", "8"], ("ris", "uniform"))
    assert core._lit_flags(["--lit", "mis:power", "a.png"]) == (["a.png"], ("mis", "power"))
    for argv, word in ((["a.png", "8", "8", "1", "--lit", "ris:power"], "ris"),
                       (["a.png", "8", "8", "1", "--lit", "ris", "--panorama"], "--panorama"),
                       (["a.png", "8", "8", "1", "cornell-box-classic", "--mis", "--lit", "ris"], "--mis"),
                       (["a.png", "8", "8", "1", "cornell-box", "--lit", "ris"], "ConstantMedium")):
        with pytest.raises(SystemExit) as ei:
            core.main(argv)
        assert word in str(ei.value), (argv, ei.value)
    with pytest.raises(AssertionError):  # a scene it does trace gets as far as the device
        core.main(["a.png", "8", "8", "1", "cornell-box-classic", "--lit", "ris", "--chunk", "2"])
    with pytest.raises(ValueError):
        refine(None, 8, 8, 4, 2, 0.1, estimator="ris", volume=True)


def _planar3(n=mcs.PLANAR_N, seed=7, control=None):
    """mis_cases.PLANAR's vertex -- the origin, normal +z -- under its three rect_xy lamps at once, each with an emission of its own, none occluding
    another (an emitter is transparent here: the scatter collects every lamp its ray crosses, so the light strategy's visibility is 1 throughout).
    -> per-sample arrays [n, 3]: light (step 5), emission (step 7 on an independent scatter), whole (that scatter's emission unweighted)"""
    table = rcs.planar3_table()
    nl = len(table)
    rng = np.random.default_rng(seed)
    K, j = rng.integers(0, 2 ** 63, n, dtype=np.uint64), np.zeros(n, np.uint64)
    p, nrm = np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1))
    d, w, m, what, live, lum = camera.ris_candidates(p, nrm, table, K, j)
    sel, S, sel_what, r, count = camera.ris_choose(what, live, K, j)
    a = np.arange(n)
    rr = np.ones(n) if control == "A" else r
    light = np.where((count > 0)[:, None], (table[sel, 7:10] * m[a, sel][:, None]) * rr[:, None], 0.0)
    emission, whole = np.zeros((n, 3)), np.zeros((n, 3))
    D = mcs.unit_ball(np.random.default_rng(seed + 2), n) + np.array([0.0, 0.0, 1.0])
    g = camera.mis_lobe(nrm, D)
    for l, (h, rect, le) in enumerate(rcs.PLANAR3):
        with np.errstate(all="ignore"):
            t = h / D[:, 2]
            x, y = t * D[:, 0], t * D[:, 1]
        hit = (D[:, 2] > 0.0) & (x >= rect[0]) & (x <= rect[2]) & (y >= rect[1]) & (y <= rect[3])
        mq = camera.mis_closing(g, nrm, D, t, table[l, 6], float(nl) if control == "B" else 1.0)[1]
        emission += np.where(hit, mq, 0.0)[:, None] * np.array(le)
        whole += hit[:, None] * np.array(le)
    return light, emission, whole, S, lum


def test_planar_identity_and_both_controls():
    """2^20 samples.  PAIRED as test_mis_host's controls are: light + emission - whole, the plain estimate taken from the same scatters as the emission
    part, must be zero within 4 standard errors of the per-sample difference, per channel and on the channel sum; control A (r dropped) and control B
    (step 7 with q = nl) must both fail that same check on the channel sum.  The light part's channel sum is S itself up to rounding: with every lamp
    visible the estimator is the sum of the proposals' shares."""
    light, emission, whole, S, lum = _planar3()
    assert np.allclose(light.sum(axis=1), S, rtol=1e-12) and (S <= lum.sum()).all() and (S > 0).any()
    for c, name in ((0, "r"), (1, "g"), (2, "b"), (None, "sum")):
        diff = (light + emission - whole)[:, c] if c is not None else (light + emission - whole).sum(axis=1)
        mean, se = _mean_se(diff)
        print("planar %s: plain %.5f, light %.5f + emission %.5f, paired difference %.5f +- %.5f (%.1f se)" % (
            name, (whole[:, c] if c is not None else whole.sum(axis=1)).mean(), (light[:, c] if c is not None else light.sum(axis=1)).mean(),
            (emission[:, c] if c is not None else emission.sum(axis=1)).mean(), mean, se, mean / se))
        assert abs(mean) <= 4.0 * se, name
    for control in ("A", "B"):
        lc, ec, wc, _, _ = _planar3(control=control)
        mean, se = _mean_se((lc + ec - wc).sum(axis=1))
        print("planar control %s: paired difference %.5f +- %.5f (%.1f se)" % (control, mean, se, mean / se))
        assert abs(mean) > 4.0 * se, control


@functools.lru_cache(maxsize=None)
def _lamps8_log(depth=3):
    o, f = _oracle(), rcs.flat("lamps8")
    lights = dref.eligible(f)
    rays, keys = rcs.view_rays(o, "lamps8"), ncs.path_keys()
    return (f, lights, rays, keys) + rref.restate(o, f, rays, keys, depth, lights, ctr0=2)


def test_the_bound_holds_on_every_contribution_and_one_lamp_is_the_mis_rule():
    """every contribution is at most T.c * (Le_sel.c / lum_sel) * sum lum (one part in 2^50 of slack for the four roundings between S and the product);
    with one lamp r is exactly 1.0 and the radiance is the MIS rule's under the uniform pick, bit for bit.  The recipes' lamps are counted first."""
    f, lights, rays, keys, rad, plain, s = _lamps8_log()
    # the recipes are what ris_cases says they are
    table = camera.light_table(f, lights)
    assert len(lights) == 8 and sorted(table[:, 0].astype(int).tolist()) == [0, 0, 0, 0, 1, 3, 4, 5]
    lum = table[:, 7:10].sum(axis=1)
    assert (lum == 0.0).sum() == 1 and len({tuple(c) for c in table[:, 7:10].tolist() if any(c)}) == 3
    fs = rcs.flat("lamps-spheres")
    ts = camera.light_table(fs, dref.eligible(fs))
    assert len(ts) == 5 and (ts[:, 0] == 0).all() and (ts[:, 7:10].sum(axis=1) == 0.0).sum() == 1
    assert len(dref.eligible(rcs.lamps32_flat())) == 32 and len(dref.eligible(rcs.lamps32_flat(33))) == 33
    i, j = s["i"], s["j"]
    got = s["contrib"][i, j]
    assert (got >= 0.0).all() and (got <= rref.bound(s, s["T"], camera.light_table(f, lights)) * (1.0 + 2.0 ** -50)).all() and got.any()
    off = int(np.flatnonzero(~s["live"])[0])  # the lamp switched off is never chosen; every other lamp is, somewhere
    assert s["live"].sum() == 7 and set(s["l"][s["built"]].tolist()) == set(range(8)) - {off}
    assert (s["count"] >= 2).any() and (s["count"] == 0).any()
    o = _oracle()
    for name in ("cornell", "sphere-lamp"):
        f1 = rcs.flat(name)
        l1 = dref.eligible(f1)
        r1, k1 = rcs.view_rays(o, name), ncs.path_keys()
        ris, _, s1 = rref.restate(o, f1, r1, k1, 3, l1, ctr0=2)
        mis, _, m1 = mref.restate(o, f1, r1, k1, 3, l1, 0, ctr0=2)
        assert len(l1) == 1 and (s1["r"][s1["built"]] == 1.0).all() and s1["built"].any()
        assert np.array_equal(rref.bits(ris), rref.bits(mis)) and np.array_equal(rref.bits(s1["d"]), rref.bits(m1["d"]))


VAR_GROUPS, VAR_N, VAR_DEPTH = 24, 256, 3


def test_the_variance_statement():
    """lamps8, fixed keys, the oracle's paths: the first 24 view rays whose first hit is Lambertian, 256 paths each, depth 3.  The summed squared standard
    error (channel sum, over the groups) of the restated proposal rule is below that of the restated MIS rule under both picks: a deterministic
    inequality.  The two ratios are printed (DESIGN.md section 7t records them)."""
    o, f = _oracle(), rcs.flat("lamps8")
    lights = dref.eligible(f)
    view = rcs.view_rays(o, "lamps8")
    rec = rcs.records(o, f, view)
    lamb = (rec[:, 0] != 0.0) & (np.asarray(f.mat_kind, np.int64)[rec[:, 11].astype(np.int64)] == 0)
    chosen = np.flatnonzero(lamb)[:VAR_GROUPS]
    assert len(chosen) == VAR_GROUPS
    rays = np.ascontiguousarray(np.repeat(view[chosen], VAR_N, axis=0))
    g, k = (a.ravel() for a in np.meshgrid(np.arange(VAR_GROUPS), np.arange(VAR_N), indexing="ij"))
    keys = util.sample_keys(0x7A12, g, k)

    def sse(rad):
        return float((rad.reshape(VAR_GROUPS, VAR_N, 3).sum(axis=2).var(axis=1, ddof=1) / VAR_N).sum())
    ris = sse(rref.restate(o, f, rays, keys, VAR_DEPTH, lights)[0])
    mis = [sse(mref.restate(o, f, rays, keys, VAR_DEPTH, lights, choice)[0]) for choice in mcs.CHOICES]
    print("summed squared standard error: ris %.6g, mis uniform %.6g (ratio %.3f), mis by power %.6g (ratio %.3f)" % (ris, mis[0], mis[0] / ris, mis[1], mis[1] / ris))
    assert ris < mis[0] and ris < mis[1]


def near_share_rows(shares):
    """the z-test of the restated rule and of its two controls against the oracle's plain paths on the near set at each share -> [(share, {rule: (mean z,
    max |z|, passes)})]"""
    o, f = _oracle(), rcs.flat("lamps8")
    lights = dref.eligible(f)
    shape = (rcs.NEAR_G, rcs.NEAR_N, 3)
    rows = []
    for share in shares:
        rays, keys = rcs.near_inputs(o, share)
        out = {}
        for control in (None, "A", "B"):
            rad, plain, _ = rref.restate(o, f, rays, keys, rcs.NEAR_DEPTH, lights, control=control)
            z = nref.z_scores(plain.reshape(shape), rad.reshape(shape))
            out[control] = (float(z.mean()), float(np.abs(z).max()), nref.same_estimand(z))
        rows.append((share, out))
    return rows


def test_near_share_row():
    """the row of ris_cases' table at NEAR_SHARE, before any device runs: the correct rule passes mis_cases' z-test, controls A and B both fail it"""
    (share, out), = near_share_rows((rcs.NEAR_SHARE,))
    for control, (mean, worst, ok) in out.items():
        print("share >= %.2f, %s: mean z %.3f (bound %.3f), max |z| %.3f" % (share, control or "correct", mean, 4.0 / math.sqrt(rcs.NEAR_G), worst))
    assert out[None][2] and not out["A"][2] and not out["B"][2]
