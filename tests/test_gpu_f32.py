"""RTMI_F32 pinned as densely as the FP64 path, and the material-record shortcuts (RTMI_TEX_CHECKER2, RTMI_TEX_GRADIENT_REC, the Dielectric's
1 / ri and r0) probed directly in both precisions.  Everything goes through the C-ABI and is compared with the CPU oracle of the same precision.

Bounds.  Float geometry and camera rays are + - * / sqrt on both sides: bit-equal.  uv passes through atan2f / asinf: the FP32 oracle lies within
1.81 * 2^-24 of the FP64 evaluation of the same float normals (5000 unit normals), the device is allowed twice the oracle's own error and a little
for the two divisions: 6 * 2^-24 (a swapped or mirrored coordinate is off by 1e-2 at least).  Paths: sinf / powf can flip a checker sign or a Schlick
draw, so at most 0.1 % of the paths may take another way (the figure test_f32_precision_matches_f32_oracle uses); the paths that do not are bit-equal
in their logs and within 4e-6 in colour (the oracle with every sinf / asinf / atan2f / powf result moved by one ulp either way changed no path of
13 x 4096 and moved rgb by 1.8e-7 at most; 4e-6 = 16 * 2^-22 over that: a handful of last-bit texture differences compounded over six segments)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import vec3
from tests.test_gpu_parity import _random_scene, random_rays, rms

UV_TOL = 6 * 2.0 ** -24
F32_COLOUR_TOL = 4 * 2.0 ** -24   # a colour of magnitude <= 1 after a few float operations
F32_LIGHT_TOL = 4 * 2.0 ** -22    # the same for emitted colours up to 4
PRECISIONS = ("f64", "f32")


def _rows_equal(a, b):
    """per row: every column bit-equal, NaN == NaN"""
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1)


def _rows_within(a, b, tol):
    with np.errstate(invalid="ignore"):
        return ((np.abs(a - b) <= tol) | (a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1)


def _check_uv(got, exp, what):
    """columns 9..10 of probe_hit on the rows that hit -> the largest uv difference (printed by the caller)"""
    hit = exp[:, 0] == 1
    err = float(np.abs(got[hit, 9:11] - exp[hit, 9:11]).max()) if hit.any() else 0.0
    assert err <= UV_TOL, "%s: uv differs from the f32 oracle by %.3g (%.2f * 2^-24)" % (what, err, err * 2.0 ** 24)
    return err


# ---- 1. the random scenes of test_random_scenes_match_oracle, in float ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_f32_random_scenes_match_f32_oracle(oracle_f32, seed):
    """Hitlist and bvh worlds, pinhole and thin-lens cameras (aperture 0 / 0.1 / 1), uv-spheres as ordinary objects, moving spheres with odd shutters,
    ri in {1.5, 2.4, 1.0, 0.7}, fuzz in {0, 0.3, 1, 10}, nested checkers at scale 37 on a radius-1000 dome, lights with gradients -- all with
    precision = "f32" against the oracle built with REAL = float, flat scan and tree."""
    f = fl.flatten(_random_scene(seed))
    nx, ny, ns = 48, 32, 6
    exp_lin, _, exp_cnt = oracle_f32.render(f, nx, ny, ns, 50, core.RENDER_SEED, nthreads=16)
    rng = np.random.default_rng(seed)
    n, n_hit = 4096, 2000
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    uv = rng.random((n, 2))
    cam = oracle_f32.probe_camera(f, uv, keys)
    rays, ctr0 = cam[:, :7], int(cam[:, 7].max())
    ehit = oracle_f32.probe_hit(f, rays[:n_hit])
    ergb, enseg, elog, enlog = oracle_f32.probe_paths(f, rays, keys, depth=50, ctr0=ctr0, max_seg=6)
    # the uv check must not be vacuous.  By the oracle, 11 of the 12 scenes send 119 .. 1774 of their 2000 camera rays onto a uv-sphere; seed 0's
    # camera looks at its ground sphere and reaches small uv-spheres in 33 rows only -- a property of that scene (the count is the oracle's own)
    on_uvsphere = int(((ehit[:, 0] == 1) & ((f.prim_kind[ehit[:, 1].astype(int)] & 15) == fl.PRIM_UVSPHERE)).sum())
    assert on_uvsphere >= (100 if seed else 30), "only %d of the camera rays end on a uv-sphere" % on_uvsphere
    ctx = core.Context(0)
    ds = core.DeviceScene(f, ctx=ctx)
    for accel in (0, 1):
        ctx.set_option("accel", accel)
        assert np.array_equal(ds.probe_camera(uv, keys, precision="f32"), cam), "accel %d: camera rays" % accel
        hit = ds.probe_hit(rays[:n_hit], precision="f32")
        assert np.array_equal(hit[:, :9], ehit[:, :9]), "accel %d: hit?, prim, t, p, normal must be bit-exact in float" % accel
        uv_err = _check_uv(hit, ehit, "seed %d accel %d" % (seed, accel))
        rgb, nseg, log, nlog = ds.probe_paths(rays, keys, depth=50, ctr0=ctr0, max_seg=6, precision="f32")
        same = nseg == enseg
        rgb_err = float(np.abs(rgb[same] - ergb[same]).max())
        lin, _, cnt = ds.render(nx, ny, ns, precision="f32")
        moved = int((np.abs(lin - exp_lin).max(axis=2) > 1e-5).sum())
        seg_diff = abs(int(cnt[0]) - int(exp_cnt[0]))
        print("seed %d accel %d: uv err %.3g (%.2f * 2^-24), paths differing %d of %d, rgb err %.3g, pixels moved %d, segments %+d, frame rms %.3g"
              % (seed, accel, uv_err, uv_err * 2.0 ** 24, int((~same).sum()), n, rgb_err, moved, int(cnt[0]) - int(exp_cnt[0]), rms(lin, exp_lin)))
        assert same.mean() >= 0.999, "accel %d: %d of %d paths took another way" % (accel, int((~same).sum()), n)
        assert np.array_equal(nlog[same], enlog[same]) and np.array_equal(log[same], elog[same]), "accel %d: segment logs" % accel
        assert rgb_err <= 4e-6, "accel %d: path colours %.3g" % (accel, rgb_err)
        assert moved <= 2, "accel %d: %d of %d pixels differ from the oracle's by more than 1e-5" % (accel, moved, nx * ny)
        assert seg_diff <= 102, "accel %d: total-rays %d vs %d" % (accel, int(cnt[0]), int(exp_cnt[0]))  # two paths' worth at depth 50
        assert cnt[1] == exp_cnt[1]
    ds.close()
    ctx.close()


# ---- 2. the Hitlist scan variants and the tree, in float ------------------------------------------------------------------------------------
def _accepted_scan_variants(ctx):
    ok = []
    for v in range(16):
        try:
            ctx.set_option("scan_variant", v)
        except core.RtmiError:
            continue
        ok.append(v)
    return ok


@pytest.mark.parametrize("moving", [False, True])
def test_f32_scan_variants_and_tree_are_bit_identical(oracle_f32, cover11, cover11_moving, moving):
    """test_scan_variants_are_bit_identical runs FP64 only: every scan variant the library accepts and the tree give the same float hits
    (uv included) and the same float frame, counters included -- and those hits are the float oracle's"""
    f = fl.flatten(cover11_moving if moving else cover11)
    rays = random_rays(20000, 31)
    exp = oracle_f32.probe_hit(f, rays)
    ctx = core.Context(0)
    ds = core.DeviceScene(f, ctx=ctx)
    variants = _accepted_scan_variants(ctx)
    assert len(variants) >= 4, variants
    first = None
    for accel in (0, 1):
        ctx.set_option("accel", accel)
        for variant in variants:
            ctx.set_option("scan_variant", variant)
            hit = ds.probe_hit(rays, precision="f32")
            img = ds.render(96, 48, 6, precision="f32")
            if first is None:
                first = (hit, img)
                assert np.array_equal(hit[:, :9], exp[:, :9])
                print("moving %s: uv err %.3g" % (moving, _check_uv(hit, exp, "cover scene")))
                assert 0.9 < exp[:, 0].mean() <= 1.0 and len(np.unique(exp[:, 1])) > 100
                continue
            assert np.array_equal(hit, first[0]), "accel %d scan_variant %d: probe_hit" % (accel, variant)
            for a, b in zip(img, first[1]):
                assert np.array_equal(a, b), "accel %d scan_variant %d: frame" % (accel, variant)
    ds.close()
    ctx.close()


# ---- 3. scatter and texture probes on the shortcut records, both precisions -------------------------------------------------------------------
def _shortcut_world():
    """one unit sphere per material, 4 apart on the x axis (the probes take the hit record as given; the emission check below aims at the lights)"""
    T, S, H = r.texture, r.shader, r.hitable
    c = lambda x, y, z: T.constant(color=vec3(x, y, z))
    grad = T.uv_gradient(co=vec3(1, .1, .2), cu=vec3(.1, 1, .3), cv=vec3(.2, .3, 1), cuv=vec3(.9, .8, .1))
    chk2 = T.checkerboard(tex0=c(.2, .3, .1), tex1=c(.9, .9, .9), scale=10.0)  # two constants: RTMI_TEX_CHECKER2 in the material record
    chkn = T.checkerboard(tex0=T.checkerboard(tex0=grad, tex1=c(.5, .5, .5), scale=37.0), tex1=grad, scale=3.0)  # nested: the generic tex_sample
    mats = [("lambertian/constant", S.lambertian(albedo=c(.4, .2, .1))), ("lambertian/checker2", S.lambertian(albedo=chk2)),
            ("lambertian/nested-checker", S.lambertian(albedo=chkn)), ("lambertian/gradient", S.lambertian(albedo=grad)),
            ("metal/constant/fuzz0", S.metal(albedo=c(.7, .6, .5), fuzz=0.0)), ("metal/gradient/fuzz.3", S.metal(albedo=grad, fuzz=0.3)),
            ("metal/checker2/fuzz1", S.metal(albedo=chk2, fuzz=1.0)), ("metal/nested-checker/fuzz10", S.metal(albedo=chkn, fuzz=10.0)),
            ("dielectric/1.5", S.dielectric(ri=1.5)), ("dielectric/2.4", S.dielectric(ri=2.4)),
            ("dielectric/1.0", S.dielectric(ri=1.0)), ("dielectric/0.7", S.dielectric(ri=0.7)),
            ("light/constant", S.diffuse_light(tex=c(4, 4, 4))), ("light/gradient", S.diffuse_light(tex=grad)),
            ("light/checker2", S.diffuse_light(tex=chk2))]
    items = [(H.uv_sphere if name.startswith("light") else H.sphere)(center=vec3(4.0 * i, 0, 0), radius=1.0, material=m)
             for i, (name, m) in enumerate(mats)]
    f = fl.flatten(H.hitlist(items=items), r.camera.PinholeCamera(*(np.zeros(3),) * 4))
    return [name for name, _ in mats], f


def _shortcut_inputs(n=8192):
    rng = np.random.default_rng(4)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o, d, time = rng.normal(size=(n, 3)), rng.normal(size=(n, 3)) * 3, rng.random((n, 1))
    d[0:512] = -nrm[0:512] * rng.uniform(0.5, 2, (512, 1))          # normal incidence from outside
    d[512:1024] = nrm[512:1024] * rng.uniform(0.5, 2, (512, 1))     # ... from inside
    tan = np.cross(nrm[1024:2048], rng.normal(size=(1024, 3))); tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    d[1024:2048] = tan + nrm[1024:2048] * rng.choice([-1e-3, -1e-6, 0.0, 1e-6, 1e-3], (1024, 1))  # grazing, either side
    d[2048:2052] = 0.0
    nrm[2560:3072] *= rng.choice([0.5, 2.0, 1e-3, 40.0], (512, 1))  # non-unit normals (a Triangle's is an un-normalised cross product)
    d[3072:3584] *= rng.choice([1e-3, 1e3], (512, 1))
    p = rng.normal(size=(n, 3)) * rng.choice([1.0, 30.0, 1000.0], (n, 1))
    p[4096:4160] = np.round(p[4096:4160])                           # sin(scale * p) = 0 at p = 0, integers elsewhere
    p[4160:4224] = np.round(p[4160:4224] / (np.pi / 10)) * (np.pi / 10)  # zeros of the scale-10 checker
    uv = rng.random((n, 2))
    uv[4224:4240] = np.tile([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]], (4, 1))
    rays = np.concatenate([o, d, time], axis=1)
    hits = np.concatenate([p, nrm, uv], axis=1)
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    return rays, hits, keys


def _holds_checker(f, t):
    """of the three in-scope texture kinds only a Checkerboard has children"""
    return f.tex_kind[t] == fl.TEX_CHECKER


def _report(name, bad, limit=8):
    idx = np.flatnonzero(bad)
    if len(idx):
        print("%s: %d rows differ: %s%s" % (name, len(idx), idx[:limit].tolist(), " ..." if len(idx) > limit else ""))
    return len(idx)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scatter_and_textures_on_shortcut_records(oracle, oracle_f32, precision):
    """probe_scatter per material and probe_texture per texture on records the host folds into the material record (a checker of two constants, a
    UVGradient, a Dielectric's 1 / ri and r0 -- FP64 reads those, RTMI_F32 computes them per hit) next to the same textures behind the generic
    tex_sample, at normal and grazing incidence from either side, a zero direction, non-unit normals, scaled directions, p on the checkers' zeros
    and uv on the corners.
    FP64: bit-equal; a Dielectric may differ in 0.05 % of the rows (xi < schlick within an ulp of the threshold) and anything holding a Checkerboard
    in 0.01 % (the 0.9995 / 0.9999 of test_scatter_matches_oracle / test_textures_match_oracle).
    FP32: scattered?, direction, time and draw count of Lambertian and Metal are bit-equal; constant and gradient colours are within 4 * 2^-24, emitted
    ones (up to 4) within 4 * 2^-22; Dielectrics and anything holding a Checkerboard may differ in 0.25 % of the rows (the float oracle with its libm
    results moved by one ulp: 0 rows of a Dielectric, at most 7 of 8192 of a checker)."""
    orc = oracle if precision == "f64" else oracle_f32
    f64 = precision == "f64"
    names, f = _shortcut_world()
    rays, hits, keys = _shortcut_inputs()
    n = len(rays)
    diel_cap, chk_cap = (0.0005, 0.0001) if f64 else (0.0025, 0.0025)
    d, nrm = rays[:, 3:6], hits[:, 3:6]
    reflected_dir = d - 2.0 * np.sum(d * nrm, axis=1, keepdims=True) * nrm  # reflect(ray-direction, normal), shader.clj:6-9
    plain = np.arange(n) >= 4240  # the rows with nothing special about them
    ds = core.DeviceScene(f)
    for i, name in enumerate(names):
        m = int(f.prim_mat[i])
        got, exp = ds.probe_scatter(m, rays, hits, keys, precision=precision), orc.probe_scatter(f, m, rays, hits, keys)
        kind, tex = int(f.mat_kind[m]), int(f.mat_tex[m])
        walk = [1, 2, 3, 7, 8]  # direction, time, draws
        if kind == fl.MAT_DIFFUSE_LIGHT:
            assert not exp.any() and not got.any(), name  # never scatters, draws nothing (column 8); its colour is checked through the paths below
            continue
        if kind == fl.MAT_DIELECTRIC:
            bad = ~_rows_equal(got, exp)
            assert _report(name, bad) <= diel_cap * n, name
            with np.errstate(invalid="ignore"):
                is_refl = np.linalg.norm(exp[:, 1:4] - reflected_dir, axis=1) <= 1e-4 * np.linalg.norm(d, axis=1)
            assert exp[:, 0].all() and (is_refl & plain).sum() > 20 and (~is_refl & plain).sum() > 20, (name, is_refl[plain].mean())
            assert set(np.unique(exp[plain, 8])) <= {0.0, 1.0}  # one draw, only where refraction is possible
            continue
        assert np.array_equal(got[:, 0], exp[:, 0]) and _rows_equal(got[:, walk], exp[:, walk]).all(), name + ": scattered?, direction, time, draws"
        if kind == fl.MAT_METAL:
            assert 0 < exp[:, 0].mean() < 1, name  # some reflected / fuzzed directions end below the surface -> nil
        else:
            assert exp[:, 0].all(), name
        colour = [4, 5, 6]
        if _holds_checker(f, tex):
            assert _report(name, ~_rows_equal(got[:, colour], exp[:, colour])) <= chk_cap * n, name
        elif f64:
            assert _report(name, ~_rows_equal(got[:, colour], exp[:, colour])) == 0, name
        else:
            assert _report(name, ~_rows_within(got[:, colour], exp[:, colour], F32_COLOUR_TOL)) == 0, name
    uvp = np.concatenate([hits[:, 6:8], hits[:, 0:3]], axis=1)
    kinds = set()
    for t in range(len(f.tex_kind)):
        got, exp = ds.probe_texture(t, uvp, precision=precision), orc.probe_texture(f, t, uvp)
        name = "texture %d (kind %d)" % (t, f.tex_kind[t])
        kinds.add(int(f.tex_kind[t]))
        if _holds_checker(f, t):
            assert _report(name, ~_rows_equal(got, exp)) <= chk_cap * n, name
        elif f64:
            assert _report(name, ~_rows_equal(got, exp)) == 0, name
        else:
            assert _report(name, ~_rows_within(got, exp, F32_COLOUR_TOL)) == 0, name
    assert kinds == {fl.TEX_CONSTANT, fl.TEX_UVGRADIENT, fl.TEX_CHECKER}
    # emitted colour of the lights' records: camera-less paths aimed at each light end on it with rgb = (sample tex uv p).  uv here is the device's
    # own (atan2f / asinf, <= 6 * 2^-24 off, times a gradient slope <= 0.9 per coordinate: 10.8 * 2^-24, plus the lerp's roundings: inside 4 * 2^-22)
    rng = np.random.default_rng(5)
    k = 2048
    for i, name in enumerate(names):
        if not name.startswith("light"):
            continue
        centre = vec3(4.0 * i, 0, 0)
        w = rng.normal(size=(k, 3)); w[:, 0] *= 0.1; w /= np.linalg.norm(w, axis=1, keepdims=True)
        o = centre + 3.0 * w
        aim = rng.normal(size=(k, 3)); aim *= (0.95 * rng.random((k, 1)) ** (1 / 3)) / np.linalg.norm(aim, axis=1, keepdims=True)
        prays = np.concatenate([o, centre + aim - o, rng.random((k, 1))], axis=1)
        pkeys = rng.integers(0, 2 ** 63, k, dtype=np.uint64)
        rgb, nseg, log, _ = ds.probe_paths(prays, pkeys, depth=50, max_seg=1, precision=precision)
        ergb, enseg, elog, _ = orc.probe_paths(f, prays, pkeys, depth=50, max_seg=1)
        assert (elog[:, 0, 0] == i).all() and (enseg == 1).all() and np.array_equal(nseg, enseg), name
        assert np.array_equal(log[:, 0, :8], elog[:, 0, :8]), name + ": prim, t, p, normal"
        shades = len(np.unique(ergb, axis=0))
        assert {"light/constant": shades == 1, "light/checker2": shades == 2, "light/gradient": shades > k // 2}[name], (name, shades)
        if "checker" in name:
            assert _report(name + " emitted", ~_rows_equal(rgb, ergb)) <= chk_cap * k, name
        else:
            err = float(np.abs(rgb - ergb).max())
            print("%s emitted: err %.3g" % (name, err))
            assert err <= (1e-12 if f64 else F32_LIGHT_TOL), (name, err)
    ds.close()


# ---- 4. RTMI_F32 is refused on mixed-kind scenes by every entry point -----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cornell", "subsurface"])
def test_f32_is_refused_on_extended_scenes_by_every_probe(scene):
    """render's refusal (-3) is checked by test_f3_scenes_match_nested_oracle; the four probes carry the same guard.  Nothing is left in flight: an
    FP64 render right after equals the one before, bit for bit."""
    sc = r.scene.make_cornell_box(16, 16) if scene == "cornell" else r.scene.make_subsurface_sphere(16, 8)
    nx, ny = (16, 16) if scene == "cornell" else (16, 8)
    rng = np.random.default_rng(8)
    n = 64
    rays = random_rays(n, 9)
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    hits = np.concatenate([rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.random((n, 2))], axis=1)
    uvp = np.concatenate([rng.random((n, 2)), rng.normal(size=(n, 3))], axis=1)
    ds = core.DeviceScene(sc)
    before = ds.render(nx, ny, 2)
    calls = {"probe_hit": lambda: ds.probe_hit(rays, precision="f32"),
             "probe_paths": lambda: ds.probe_paths(rays, keys, depth=5, max_seg=2, precision="f32"),
             "probe_texture": lambda: ds.probe_texture(0, uvp, precision="f32"),
             "probe_scatter": lambda: ds.probe_scatter(0, rays, hits, keys, precision="f32")}
    for name, call in calls.items():
        with pytest.raises(core.RtmiError) as e:
            call()
        assert e.value.code == -3, (name, e.value.code)
        after = ds.render(nx, ny, 2)
        for a, b in zip(before, after):
            assert np.array_equal(a, b), name
    assert before[2][1] == nx * ny and before[0].any()
    ds.close()
