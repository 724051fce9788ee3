"""The feature pass (rtmi_render_features*) and the denoiser (rtmi_denoise*) on the device.

  * Features bit for bit against a composition of the oracle's probes (denoise_reference.feature_samples) for the libm-free scenes of
    frame_reference, f64 and f32; within the image-parity RMS bound for the cover scene (uv through asin / atan2); through probe_paths for a
    world with media.
  * An independent route for thin lens and moving spheres: a copy of the scene whose materials are all DiffuseLights of their albedo texture
    renders, through the existing path, exactly the albedo plane.
  * The features do not depend on region, accel, suspend_lanes or flat_below, the device form equals the host form, and a live progressive or
    adaptive frame is not disturbed.
  * The filter bit for bit against denoise_reference.denoise (numpy, written from the header): every term alone and all together, missing inputs,
    inf / NaN pixels, 0 passes, the 8-bit frame.
  * The filter helps: at 16 spp the filtered frame is closer to a 4096-spp frame than the raw one.
Every comparison is an equality except where a docstring derives its bound."""
import copy
import re

import numpy as np
import pytest

import denoise_reference as dr
import frame_reference as fr
import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import vec3

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-13  # the bound of the image parity tests (test_gpu_parity.py)
NAS = (1, 2, 7)
MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT = 2, 3
SIGMAS = dict(sigma_c=2.0, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


# ---- features against the oracle, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("spheres", "f64"), ("spheres", "f32"), ("mixed", "f64")])
def test_features_equal_the_oracle_composition(request, ctx, name, precision):
    o = _oracle(request, precision)
    nx, ny = fr.SIZE
    flat = fr.scene(name, nx, ny)
    smp = dr.feature_samples(o, flat, nx, ny, max(NAS))
    assert 0.2 < smp[..., 7].mean() <= 1.0 and len(np.unique(smp[..., 0])) > 10
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        for accel in (1, 0):
            ctx.set_option("accel", accel)
            for na in NAS:
                ft, cnt = ds.render_features(nx, ny, na, seed=fr.SEED, precision=precision)
                ref = dr.feature_frame(smp, na)
                bad = (ft != ref).any(axis=2)
                print("%s %s accel %d na %d: %d of %d pixels differ" % (name, precision, accel, na, bad.sum(), bad.size))
                assert np.array_equal(ft, ref), (name, precision, accel, na, int(bad.sum()))
                assert list(cnt) == [nx * ny * na, nx * ny]
    finally:
        ctx.set_option("accel", 1)
        ds.close()


def test_features_of_a_frame_of_many_workgroups(oracle, ctx):
    nx, ny = fr.SIZE_PASSES["spheres"]  # 26 x 13 tiles: 85 workgroups of four waves
    flat = fr.scene("spheres", nx, ny)
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        ft, cnt = ds.render_features(nx, ny, 2, seed=fr.SEED)
        assert np.array_equal(ft, dr.feature_frame(dr.feature_samples(oracle, flat, nx, ny, 2)))
        assert list(cnt) == [nx * ny * 2, nx * ny]
    finally:
        ds.close()


def test_features_in_a_world_with_media(oracle, ctx):
    """A pinhole view of the foggy Cornell box: prim, t, p and normal of segment 0 from the oracle's probe_paths with the stream at draw 2.
    A medium's free-flight distance goes through log (ocml against glibc, <= 1 ulp), so t and p of a medium hit may differ in the last bits and a
    distance that lands within an ulp of the chord may flip one hit: as in test_media_match_oracle, pixels whose coverage agrees must be
    99.9 % of the frame, and on them the albedo (constants) is equal and normal and depth agree to 1e-9."""
    from oracle.tree import attach_tree
    nx, ny = 48, 40
    sc = r.scene.make_cornell_box(nx, ny, classic=False)
    cam = r.camera.pinhole_camera(lookfrom=vec3(278, 278, -800), lookat=vec3(278, 278, 0), vup=vec3(0, 1, 0), vfov=40, aspect=nx / ny)
    flat = attach_tree(fl.flatten({"camera": cam, "world": sc["world"]}), sc["world"])
    media = np.flatnonzero((np.asarray(flat.prim_kind) & 15) == 7)
    assert len(media) == 2
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        for na in (1, 3):
            smp = dr.feature_samples_media(oracle, flat, nx, ny, na)
            ref = dr.feature_frame(smp)
            for accel in (1, 0):
                ctx.set_option("accel", accel)
                ft, _ = ds.render_features(nx, ny, na, seed=fr.SEED)
                same = ft[..., 7] == ref[..., 7]
                print("media na %d accel %d: coverage agrees in %.4f of the pixels" % (na, accel, same.mean()))
                assert same.mean() > 0.999
                close = np.isclose(ft, ref, rtol=1e-9, atol=1e-9).all(axis=2)
                assert close[same].mean() > 0.999, "a flipped medium hit moves one pixel, not many"
                if na == 1:
                    assert np.array_equal(ft[same & close][:, 0:3], ref[same & close][:, 0:3])
        # media are actually hit at segment 0, with the Isotropic's constant as albedo: white fog (1 1 1) and black smoke (0 0 0)
        one = dr.feature_samples_media(oracle, flat, nx, ny, 1)[:, :, 0]
        keys, rays = dr.sample_rays(oracle, flat, nx, ny, 1)
        _, _, log, nlog = oracle.probe_paths(flat, rays, keys, depth=fr.DEPTH, ctr0=2, max_seg=1)
        in_medium = (nlog > 0) & np.isin(log[:, 0, 0], media)
        assert in_medium.sum() > 50
        alb = one.reshape(-1, 8)[in_medium][:, 0:3]
        assert set(map(tuple, np.unique(alb, axis=0))) == {(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)}
    finally:
        ctx.set_option("accel", 1)
        ds.close()


# ---- an independent route: the albedo plane through the existing render path ---------------------------------------------------------------------
def as_lights(flat):
    """a copy of the scene with every material replaced by a DiffuseLight of its albedo texture (a Dielectric: of a constant (1 1 1)): a path
    ends on its first hit with emitted = the texture there, so render(ns) is the mean of the first-hit albedo over samples 0 .. ns-1"""
    f = copy.copy(flat)
    kind, tex = np.array(flat.mat_kind, np.int32), np.array(flat.mat_tex, np.int32)
    if (kind == MAT_DIELECTRIC).any():
        ones = np.zeros((1, flat.tex_param.shape[1]))
        ones[0, 0:3] = 1.0
        tex[kind == MAT_DIELECTRIC] = len(flat.tex_kind)
        f.tex_kind = np.concatenate([flat.tex_kind, [0]]).astype(np.int32)
        f.tex_param = np.concatenate([flat.tex_param, ones])
        f.tex_child = np.concatenate([flat.tex_child, [[-1, -1]]]).astype(np.int32)
    f.mat_kind = np.full_like(kind, MAT_DIFFUSE_LIGHT)
    f.mat_tex = tex
    return f


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_albedo_plane_equals_a_render_of_lights_thin_lens_and_moving_spheres(ctx, precision):
    nx, ny = fr.SIZE
    flat = fr.scene("spheres-lens", nx, ny)
    assert int(flat.cam_kind) == 1 and ((np.asarray(flat.prim_kind) & 15) == 2).any()
    ds, lights = core.DeviceScene(flat, ctx=ctx), core.DeviceScene(as_lights(flat), ctx=ctx)
    try:
        for na in NAS:
            ft, _ = ds.render_features(nx, ny, na, seed=fr.SEED, precision=precision)
            lin, _, cnt = lights.render(nx, ny, na, fr.DEPTH, fr.SEED, precision)
            assert int(cnt[0]) == nx * ny * na, "one segment per sample"
            assert np.array_equal(ft[..., 0:3], lin), (precision, na, int((ft[..., 0:3] != lin).any(axis=2).sum()))
            ft2, _ = lights.render_features(nx, ny, na, seed=fr.SEED, precision=precision)
            assert np.array_equal(ft2, ft), "the geometry and the textures are the same scene's"
        assert len(np.unique(ft[..., 0])) > 20 and 0 < ft[..., 7].mean() <= 1
    finally:
        ds.close()
        lights.close()


def test_albedo_plane_equals_a_render_of_lights_cover_scene_at_c2_size(ctx):
    """the cover scene (thin-lens camera, moving spheres, entry grid) at 800 x 400 through the tree and the flat scan"""
    nx, ny, na = 800, 400, 2
    flat = fl.flatten(r.scene.make_random_scene(nx, ny, 11, True))
    ds, lights = core.DeviceScene(flat, ctx=ctx), core.DeviceScene(as_lights(flat), ctx=ctx)
    try:
        got = {}
        for accel in (1, 0):
            ctx.set_option("accel", accel)
            got[accel], _ = ds.render_features(nx, ny, na)
        assert np.array_equal(got[0], got[1])
        ctx.set_option("accel", 1)
        lin, _, _ = lights.render(nx, ny, na)
        diff = (got[1][..., 0:3] != lin).any(axis=2)
        print("cover C2: %d of %d pixels differ from the render of lights, largest difference %.3g" % (diff.sum(), diff.size, np.abs(got[1][..., 0:3] - lin).max()))
        assert np.array_equal(got[1][..., 0:3], lin), int(diff.sum())
    finally:
        ctx.set_option("accel", 1)
        ds.close()
        lights.close()


def test_cover_scene_features_match_the_oracle(oracle, ctx, cover_small):
    """uv spheres: u and v go through atan2 / asin, where device and libm may differ in the last bits: the RMS bound of the image parity tests"""
    nx, ny, na = 96, 48, 3
    cam = r.camera.pinhole_camera(lookfrom=vec3(13, 2, 3), lookat=vec3(0, 0, 0), vup=vec3(0, 1, 0), vfov=20, aspect=nx / ny)
    flat = fl.flatten({"camera": cam, "world": cover_small["world"]})
    ref = dr.feature_frame(dr.feature_samples(oracle, flat, nx, ny, na))
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        for accel in (1, 0):
            ctx.set_option("accel", accel)
            ft, _ = ds.render_features(nx, ny, na, seed=fr.SEED)
            print("cover features accel %d: RMS %.3g, %d values differ" % (accel, dr.rms(ft, ref), (ft != ref).sum()))
            assert dr.rms(ft, ref) <= RMS_TOL
            assert np.array_equal(ft[..., 7], ref[..., 7])
    finally:
        ctx.set_option("accel", 1)
        ds.close()


# ---- invariance -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spheres-lens", "mixed"])
def test_features_do_not_depend_on_region_or_options(name):
    nx, ny = fr.SIZE
    na = 3
    c = core.Context(0)
    ds = core.DeviceScene(fr.scene(name, nx, ny), ctx=c)
    try:
        whole, cnt = ds.render_features(nx, ny, na, seed=fr.SEED)
        for rg in [(5, 3, 50, 30), (13, 0, 61, 21), (8, 8, 9, 9), (0, 0, 8, 8)]:
            part, pc = ds.render_features(nx, ny, na, seed=fr.SEED, region=rg)
            x0, y0, x1, y1 = rg
            assert np.array_equal(part, whole[y0:y1, x0:x1]), rg
            assert list(pc) == [(x1 - x0) * (y1 - y0) * na, (x1 - x0) * (y1 - y0)]
        for opt, values in (("accel", (0, 1)), ("suspend_lanes", (0, 24, 8)), ("flat_below", (0, 1000, 24)), ("scan_variant", (0, 1, 2, 3))):
            for v in values:
                c.set_option(opt, v)
                for accel in ((0, 1) if opt != "accel" else (v,)):
                    c.set_option("accel", accel)
                    assert np.array_equal(ds.render_features(nx, ny, na, seed=fr.SEED)[0], whole), (opt, v, accel)
            c.set_option("accel", 1)
    finally:
        ds.close()
        c.close()


def test_device_form_equals_host_form(ctx):
    torch = pytest.importorskip("torch")
    nx, ny, na = fr.SIZE[0], fr.SIZE[1], 3
    ds = core.DeviceScene(fr.scene("spheres-lens", nx, ny), ctx=ctx)
    try:
        for precision in ("f64", "f32"):
            host, hcnt = ds.render_features(nx, ny, na, seed=fr.SEED, precision=precision)
            st = torch.cuda.Stream()
            out = torch.full((ny, nx, 8), -1.0, dtype=torch.float64, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ds.render_features_device(nx, ny, na, out, cnt, seed=fr.SEED, precision=precision, stream=st.cuda_stream)
            st.synchronize()
            assert np.array_equal(out.cpu().numpy(), host) and list(cnt.cpu().numpy()) == list(hcnt.astype(np.int64))
            out.fill_(-1.0)
            torch.cuda.synchronize()
            ds.render_features_device(nx, ny, na, out, None, seed=fr.SEED, precision=precision)  # the context's own stream, no counters
            ds.render_features(nx, ny, 1, seed=fr.SEED, region=(0, 0, 8, 8))  # a host call on the same context synchronises that stream
            assert np.array_equal(out.cpu().numpy(), host)
    finally:
        ds.close()


def test_a_live_progressive_or_adaptive_frame_is_not_disturbed():
    nx, ny = fr.SIZE
    c = core.Context(0)
    ds = core.DeviceScene(fr.scene("spheres-lens", nx, ny), ctx=c)
    try:
        ref = [ds.render(nx, ny, k, fr.DEPTH, fr.SEED) for k in (3, 5, 9)]
        ft = ds.render_features(nx, ny, 2, seed=fr.SEED)[0]
        for k0, n, want in ((0, 3, ref[0]), (3, 2, ref[1]), (5, 4, ref[2])):
            lin, q, err, cnt = ds.render_progressive(nx, ny, k0, n, fr.DEPTH, fr.SEED)
            assert np.array_equal(lin, want[0]) and np.array_equal(q, want[1]) and np.array_equal(cnt, want[2])
            assert np.array_equal(ds.render_features(nx, ny, 2, seed=fr.SEED)[0], ft)
            assert np.array_equal(ds.render_features(nx, ny, 1, seed=fr.SEED, region=(3, 3, 20, 20))[0].shape, (17, 17, 8))
            c.denoise(lin, err, ft, iterations=2, **SIGMAS)
            assert c.progressive_samples() == k0 + n
        # adaptive: the same sequence of calls with and without feature / denoise calls in between
        eps = float(np.quantile(err, 0.8))
        plain = [ds.render_adaptive(nx, ny, k0, n, eps, fr.DEPTH, fr.SEED) for k0, n in ((0, 4), (4, 4), (8, 4))]
        status = c.adaptive_status()
        print("adaptive frame: %d of %d tiles active after 12 samples" % status[:2])
        for i, (k0, n) in enumerate(((0, 4), (4, 4), (8, 4))):
            got = ds.render_adaptive(nx, ny, k0, n, eps, fr.DEPTH, fr.SEED)
            assert all(np.array_equal(a, b) for a, b in zip(got, plain[i])), i
            assert np.array_equal(ds.render_features(nx, ny, 2, seed=fr.SEED)[0], ft)
            c.denoise(got[0], got[2], ft, iterations=1, **SIGMAS)
        assert c.adaptive_status() == status
    finally:
        c.progressive_release()
        ds.close()
        c.close()


# ---- the filter against the numpy reference, bit for bit ------------------------------------------------------------------------------------------
TERMS = {"colour": dict(sigma_c=2.0), "normal": dict(sigma_n=0.3), "albedo": dict(sigma_a=0.1), "depth": dict(sigma_d=0.1), "all": SIGMAS,
         "none": {}}


def _check_filter(ctx, lin, se, ft, iterations, sig, what):
    zero = dict(sigma_c=0.0, sigma_n=0.0, sigma_a=0.0, sigma_d=0.0)
    kw = dict(zero, **sig)
    got = ctx.denoise(lin, se, ft, iterations=iterations, **kw)
    exp = dr.denoise(lin, se, ft, iterations=iterations, **kw)
    for g, e, n in zip(got, exp, ("linear", "rgb8", "stderr")):
        bad = g != e
        if g.dtype != np.uint8:
            bad &= ~(np.isnan(g) & np.isnan(e))
        assert not bad.any(), (what, n, "%d of %d values differ" % (bad.sum(), bad.size))
    assert np.array_equal(got[1], fr.quantise(got[0]))
    return got


@pytest.mark.parametrize("size", [(61, 37), (203, 99)])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_equals_the_numpy_reference(ctx, size, iterations):
    nx, ny = size
    lin, se, ft = dr.synthetic_frame(nx, ny, seed=nx)
    outs = {}
    for term, sig in TERMS.items():
        outs[term] = _check_filter(ctx, lin, se, ft, iterations, sig, (size, iterations, term))[0]
    for term in ("colour", "normal", "albedo", "depth", "all"):
        assert not np.array_equal(outs[term], outs["none"]), "the %s term changes the result" % term
    _check_filter(ctx, lin, None, ft, iterations, SIGMAS, (size, iterations, "stderr=None"))
    _check_filter(ctx, lin, se, None, iterations, SIGMAS, (size, iterations, "features=None"))
    _check_filter(ctx, lin, None, None, iterations, SIGMAS, (size, iterations, "no guide at all"))


def test_filter_with_inf_and_nan_pixels_and_zero_iterations(ctx):
    nx, ny = 61, 37
    lin, se, ft = dr.synthetic_frame(nx, ny, seed=9)
    lin[5, 5] = np.nan
    lin[20, 40, 1] = np.inf
    lin[30, 10, 2] = -np.inf
    lin[0, 0, 0] = np.inf
    se[10:14, 20:24] = np.inf  # one-sample pixels
    se[8, 8] = np.nan
    se[16:18, 3:9] = 0.0       # pixels whose samples were all equal
    ft[25, 50, 6] = np.nan
    for iterations in (1, 4, 8):
        for term in ("colour", "all", "none"):
            out, q, err = _check_filter(ctx, lin, se, ft, iterations, TERMS[term], (iterations, term, "inf / NaN"))
            for y, x in ((5, 5), (20, 40), (30, 10), (0, 0)):
                assert np.array_equal(out[y, x], lin[y, x], equal_nan=True)
            ok = np.isfinite(lin).all(axis=2)
            assert np.isfinite(out[ok]).all()
    for se_in, ft_in in ((se, ft), (None, None), (se, None)):
        out, q, err = ctx.denoise(lin, se_in, ft_in, iterations=0, **SIGMAS)
        assert out.tobytes() == lin.tobytes(), "0 passes copy the frame bit for bit"
        assert err.tobytes() == (se if se_in is not None else np.zeros_like(se)).tobytes()
        assert np.array_equal(q, fr.quantise(lin))


def test_filter_device_form_equals_host_form(ctx):
    torch = pytest.importorskip("torch")
    nx, ny = 203, 99
    lin, se, ft = dr.synthetic_frame(nx, ny, seed=4)
    host = ctx.denoise(lin, se, ft, iterations=3, **SIGMAS)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_lin, d_se, d_ft = (torch.from_numpy(a).cuda() for a in (lin, se, ft))
        o_lin, o_se = torch.zeros_like(d_lin), torch.zeros_like(d_se)
        o_q = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
    st.synchronize()
    ctx.denoise_device(nx, ny, d_lin, d_se, d_ft, o_lin, o_q, o_se, iterations=3, stream=st.cuda_stream, **SIGMAS)
    st.synchronize()
    for g, e in zip((o_lin, o_q, o_se), host):
        assert np.array_equal(g.cpu().numpy(), e)
    ctx.denoise_device(nx, ny, d_lin, d_se, d_ft, d_lin, None, d_se, iterations=3, stream=st.cuda_stream, **SIGMAS)  # in place, rgb8 not wanted
    st.synchronize()
    assert np.array_equal(d_lin.cpu().numpy(), host[0]) and np.array_equal(d_se.cpu().numpy(), host[2])


# ---- it must help ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cover", "cornell"])
def test_filtered_frame_is_closer_to_the_truth(ctx, which):
    """16 spp, the library's default passes and sigmas, against a 4096-spp one-shot render on the existing path: strictly smaller RMS error"""
    if which == "cover":
        nx, ny = 200, 100
        sc = r.scene.make_random_scene(nx, ny, 3, False)
    else:
        nx, ny = 128, 128
        sc = r.scene.make_cornell_box(nx, ny)
    ds = core.DeviceScene(sc, ctx=ctx)
    try:
        truth, _, _ = ds.render(nx, ny, 4096, seed=core.RENDER_SEED + 1)
        raw, ft, (flt, q, err) = ds.render_denoised(nx, ny, 16)
        assert np.array_equal(raw[0], ds.render(nx, ny, 16)[0]), "the raw frame is the one-shot frame"
        e_raw, e_flt = dr.rms(raw[0], truth), dr.rms(flt, truth)
        print("%s 16 spp: RMS error raw %.5f filtered %.5f ratio %.3f; mean stderr raw %.5f filtered %.5f" % (
            which, e_raw, e_flt, e_flt / e_raw, raw[2].mean(), err.mean()))
        assert e_flt < e_raw
        assert np.array_equal(q, fr.quantise(flt))
    finally:
        ctx.progressive_release()
        ds.close()


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------------
def _progress_lines(text):
    return [l for l in text.splitlines() if re.fullmatch(r"\d+\.\d\ds, \d+%, ETA -?\d+\.\d\ds", l)]


def _ppm(path, nx, ny):
    head = b"P6\n%d %d\n255\n" % (nx, ny)
    data = path.read_bytes()
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(ny, nx, 3)


def test_cli_denoise(tmp_path, capsys):
    nx, ny = 64, 32
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"
    assert core.main([str(a), "64", "32", "10"]) == 0
    plain_text = capsys.readouterr().out
    assert not (tmp_path / "a.denoised.ppm").exists()
    assert core.main([str(b), "64", "32", "10", "--denoise"]) == 0
    text = capsys.readouterr().out
    assert a.read_bytes() == b.read_bytes(), "the unfiltered file is the plain run's"
    assert len(_progress_lines(text)) == len(_progress_lines(plain_text)) == 1
    assert [l for l in text.splitlines() if l.startswith("total-rays")] == [l for l in plain_text.splitlines() if l.startswith("total-rays")]
    assert ("wrote %s" % (tmp_path / "b.denoised.ppm")) in text
    ds = core.DeviceScene(r.scene.make_random_scene(nx, ny, 11, True))
    try:
        raw, ft, flt = ds.render_denoised(nx, ny, 10)
        assert np.array_equal(_ppm(b, nx, ny), raw[1]) and np.array_equal(_ppm(tmp_path / "b.denoised.ppm", nx, ny), flt[1])
        assert not np.array_equal(flt[1], raw[1])
        # passes and feature samples as given; with --chunk the frame is the same frame
        assert core.main([str(b), "64", "32", "10", "--denoise", "2", "--feature-samples", "1", "--chunk", "4"]) == 0
        text = capsys.readouterr().out
        assert len(_progress_lines(text)) == 3
        raw2, ft2, flt2 = ds.render_denoised(nx, ny, 10, na=1, iterations=2)
        assert np.array_equal(_ppm(b, nx, ny), raw[1]) and np.array_equal(_ppm(tmp_path / "b.denoised.ppm", nx, ny), flt2[1])
        # --denoise 0: the filtered file is the unfiltered one
        assert core.main([str(b), "64", "32", "10", "--denoise=0"]) == 0
        capsys.readouterr()
        assert (tmp_path / "b.denoised.ppm").read_bytes() == b.read_bytes()
        # with --adaptive: the unfiltered file is the adaptive run's, the filtered one is the filter of that frame
        c = tmp_path / "c.ppm"
        assert core.main([str(c), "64", "32", "32", "--adaptive", "0.05", "--chunk", "8"]) == 0
        plain_text = capsys.readouterr().out
        assert core.main([str(b), "64", "32", "32", "--adaptive", "0.05", "--chunk", "8", "--denoise"]) == 0
        text = capsys.readouterr().out
        assert c.read_bytes() == b.read_bytes()
        keep = lambda t: [l for l in t.splitlines() if l.startswith(("samples:", "total-rays"))]
        assert keep(text) == keep(plain_text) and len(_progress_lines(text)) == len(_progress_lines(plain_text))
        got = list(ds.refine_adaptive(nx, ny, 32, 8, 0.05))[-1]
        ft = ds.render_features(nx, ny, core.FEATURE_SAMPLES)[0]
        assert np.array_equal(_ppm(tmp_path / "b.denoised.ppm", nx, ny), ds.ctx.denoise(got[1], got[3], ft)[1])
    finally:
        ds.ctx.progressive_release()
        ds.close()
