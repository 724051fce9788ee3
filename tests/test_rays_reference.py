"""CPU side of rtmi_render_rays: the restated fold (rays_reference.py) against the oracle's own frame, the chunk rule, the edges of the noise
estimate, the ray generators of camera.py, and the condition on its input that makes the GPU refill test mean something."""
import numpy as np
import pytest

import depth_cases as dc
import frame_reference as fr
import rays_reference as rr
import raytrace_clj_amd as r
from raytrace_clj_amd import camera as cam


def test_grouped_probe_paths_are_the_oracles_frame(oracle):
    """per-pixel groups of the oracle's probe_paths colours, folded by the restatement = Oracle.render's linear frame, bit for bit"""
    nx, ny, ns = 16, 8, 5
    f = dc.flat("cover")
    rays, keys, ctr = dc.frame_paths(lambda uv, k: oracle.probe_camera(f, uv, k), f, nx, ny, ns)
    rgb, nseg, _, _ = dc.probe_frame_paths(lambda *a, **kw: oracle.probe_paths(f, *a, **kw), rays, keys, ctr, dc.FULL)
    mean, err = rr.fold(rr.pixel_major(rgb, nx, ny, ns), ns)
    lin, _, cnt = oracle.render(f, nx, ny, ns, dc.FULL, dc.SEED)
    assert np.array_equal(mean.reshape(ny, nx, 3), lin)
    assert int(nseg.sum()) == int(cnt[0])
    assert np.isfinite(err).all() and (err > 0).any()


def _samples(n_groups, group, precision, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.random((n_groups * group, 3)) * rng.choice([1e-3, 1.0, 40.0], (n_groups * group, 1))
    return x.astype(fr.REAL[precision]).astype(np.float64)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("split", [(5, 7), (1, 1, 10), (12,), (1,) * 12, (11, 1)])
def test_any_split_into_chunks_is_the_one_shot(precision, split):
    ng, group = 37, 12
    x = _samples(ng, group, precision).reshape(ng, group, 3)
    want = rr.fold(x.reshape(-1, 3), group, precision)
    state, first = rr.new_state(ng), 0
    for n in split:
        got = rr.fold(x[:, first:first + n].reshape(-1, 3), n, precision, first, state)
        first += n
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    whole = rr.new_state(ng)
    rr.fold(x.reshape(-1, 3), group, precision, 0, whole)
    assert np.array_equal(state, whole) and (state[:, 9] == group).all()
    # the restatement is the frame's: sums and means of fold_in_order / mean_of, the two-pass standard error within rounding
    smp = x.reshape(ng, 1, group, 3).astype(fr.REAL[precision])
    assert np.array_equal(want[0], fr.mean_of(fr.fold_in_order(smp), group).reshape(ng, 3).astype(np.float64))
    assert np.allclose(want[1], fr.stderr_two_pass(smp, group).ravel(), rtol=1e-9, atol=0)


def test_a_state_continues_only_with_its_count():
    state = rr.new_state(2)
    rr.fold(_samples(2, 3, "f64"), 3, "f64", 0, state)
    with pytest.raises(AssertionError):
        rr.fold(_samples(2, 3, "f64"), 3, "f64", 2, state)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_noise_estimate_edges(precision):
    x = _samples(9, 1, precision)
    mean, err = rr.fold(x, 1, precision)
    assert np.array_equal(mean, x) and np.isposinf(err).all()            # count == 1: the ray itself, +inf
    state = rr.new_state(9)
    assert np.isposinf(rr.fold(x, 1, precision, 0, state)[1]).all()
    assert np.isfinite(rr.fold(x, 1, precision, 1, state)[1]).all()      # ... and finite from the second ray on
    same = np.repeat(np.array([[0.1, 0.7, 3.3], [0.0, 1e-30, 1e30]]).astype(fr.REAL[precision]).astype(np.float64), 7, axis=0)
    mean, err = rr.fold(same, 7, precision)
    assert (err == 0.0).all()                                            # equal samples: exactly 0, whatever sum * (1 / 7) rounds to
    assert not np.array_equal(rr.fold(_samples(4, 7, precision), 7, precision)[1], np.zeros(4))


def test_derived_keys_are_sample_keys():
    k = rr.derived_keys(0xABCDEF0012345678, 3, 4, 5)
    for g in range(3):
        for s in range(4):
            assert int(k[g * 4 + s]) == r.util.sample_key(0xABCDEF0012345678, g, 5 + s)
    assert np.array_equal(r.util.sample_keys(7, np.arange(5), 2), fr.sample_keys(7, np.arange(5), 2))
    assert np.array_equal(r.util.draw_uniforms(k, 1), fr.draws(k, 1, "f64"))


# ---- the ray generators ------------------------------------------------------------------------------------------------------------------------
LOOK = dict(lookfrom=np.array([278.0, 278.0, 278.0]), lookat=np.array([278.0, 278.0, 500.0]), vup=np.array([0.0, 1.0, 0.0]))


def _unit(d):
    return np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() < 1e-14


def test_panorama_rays():
    nx, ny, ns = 32, 16, 3
    rays, ctr0 = cam.panorama_rays(nx, ny, 0, ns, **LOOK)
    assert rays.shape == (nx * ny * ns, 7) and ctr0 == 2 and (rays[:, 6] == 0.0).all()
    assert (rays[:, :3] == LOOK["lookfrom"]).all() and _unit(rays[:, 3:6])
    d = rays[:, 3:6].reshape(ny, nx, ns, 3)                              # [j, i, s]: j = 0 is the bottom row
    fwd = np.array([0.0, 0.0, 1.0])
    pixel = np.hypot(2 * np.pi / nx, np.pi / ny)                         # no direction of a pixel is further from its centre than this
    for i in (nx // 2 - 1, nx // 2):
        for j in (ny // 2 - 1, ny // 2):                                 # the four pixels around the image centre look forward
            assert (np.arccos(np.clip(d[j, i] @ fwd, -1, 1)) <= pixel).all()
    assert (np.arccos(np.clip(d[ny - 1] @ LOOK["vup"], -1, 1)) <= np.pi / ny + 1e-12).all()     # top row: within one row of +vup
    assert (np.arccos(np.clip(d[0] @ -LOOK["vup"], -1, 1)) <= np.pi / ny + 1e-12).all()         # bottom row: of -vup
    octants = {tuple(s) for s in (rays[:, 3:6] > 0).astype(int)}
    assert len(octants) == 8
    # longitude grows to the right of the view: the column right of the centre lies on the side of forward x up
    assert (d[ny // 2, nx // 2 + 3] @ np.cross(fwd, LOOK["vup"]) > 0).all()
    # a chunk is the slice of the longer run
    a, b = 2, 7
    part, _ = cam.panorama_rays(nx, ny, a, b - a, **LOOK)
    whole, _ = cam.panorama_rays(nx, ny, 0, b, **LOOK)
    assert np.array_equal(part, whole.reshape(nx * ny, b, 7)[:, a:b].reshape(-1, 7))
    assert not np.array_equal(cam.panorama_rays(nx, ny, 0, ns, seed=1, **LOOK)[0], rays)
    with pytest.raises(ValueError):
        cam.panorama_rays(nx, 0, 0, 1, **LOOK)


def test_panorama_jitter_is_the_streams_first_two_draws():
    nx, ny = 8, 4
    rays, _ = cam.panorama_rays(nx, ny, 3, 2, seed=99, **LOOK)
    pix, ss = (a.ravel() for a in np.meshgrid(np.arange(nx * ny), np.arange(3, 5), indexing="ij"))
    keys = fr.sample_keys(99, pix, ss)
    lon = ((pix % nx + fr.draws(keys, 0, "f64")) / nx - 0.5) * 2 * np.pi
    lat = ((pix // nx + fr.draws(keys, 1, "f64")) / ny - 0.5) * np.pi
    assert np.allclose(rays[:, 4], np.sin(lat), rtol=0, atol=1e-15)
    assert np.allclose(np.arctan2(rays[:, 3], rays[:, 5]), -lon, rtol=0, atol=1e-12) or np.allclose(np.arctan2(-rays[:, 3], rays[:, 5]), lon, rtol=0, atol=1e-12)


def test_orthographic_rays():
    nx, ny, ns = 12, 6, 2
    look = dict(lookfrom=np.array([3.0, 2.0, 1.0]), lookat=np.array([0.0, 0.5, 0.0]), vup=np.array([0.0, 1.0, 0.0]))
    rays, ctr0 = cam.orthographic_rays(nx, ny, 0, ns, width=4.0, **look)
    assert rays.shape == (nx * ny * ns, 7) and ctr0 == 2
    d = look["lookat"] - look["lookfrom"]
    d /= np.linalg.norm(d)
    assert (rays[:, 3:6] == rays[0, 3:6]).all() and np.allclose(rays[0, 3:6], d, atol=1e-15) and _unit(rays[:, 3:6])   # parallel
    off = rays[:, :3] - look["lookfrom"]
    assert np.abs(off @ d).max() < 1e-14                                                                              # origins in the plane
    right = np.cross(d, look["vup"])
    right /= np.linalg.norm(right)
    x, y = off @ right, off @ np.cross(right, d)
    assert -2.0 <= x.min() < -1.6 and 1.6 < x.max() <= 2.0 and -1.0 <= y.min() < -0.6 and 0.6 < y.max() <= 1.0        # the window, width x width ny / nx
    o = rays[:, :3].reshape(ny, nx, ns, 3)
    assert ((o[:, 1:] - o[:, :-1]) @ right > -4.0 / nx).all() and ((o[-1] - o[0]) @ np.cross(right, d) > 0).all()    # i to the right, j upwards
    part, _ = cam.orthographic_rays(nx, ny, 1, 3, width=4.0, **look)
    whole, _ = cam.orthographic_rays(nx, ny, 0, 4, width=4.0, **look)
    assert np.array_equal(part, whole.reshape(nx * ny, 4, 7)[:, 1:4].reshape(-1, 7))


# ---- the refill test's input -------------------------------------------------------------------------------------------------------------------
def test_refill_rays_diverge_for_the_oracle(oracle):
    """at least a tenth of the rays end at their first segment and at least a tenth run four segments or more: neighbouring lanes of a wave finish
    far apart, so a kernel that never deals a lane a second ray cannot pass test_gpu_rays.py's refill test"""
    rays, keys, ctr0 = rr.refill_base(oracle)
    _, nseg, _, _ = oracle.probe_paths(rr.glass_flat(), rays, keys, depth=dc.FULL, ctr0=ctr0)
    assert (nseg[1::2] == 1).all()                    # the rays that miss everything
    assert (nseg == 1).mean() >= 0.1 and (nseg >= 4).mean() >= 0.1, ((nseg == 1).mean(), (nseg >= 4).mean())
    big, _, _ = rr.refill_set(oracle, 3 * len(rays) - 5)
    assert len(big) == 3 * len(rays) and np.array_equal(big[len(rays):2 * len(rays)], rays)


def test_pinhole_copies_keep_the_image_plane():
    for name in rr.SCENES:
        f, g = dc.flat(name), rr.pinhole_flat(name)
        assert int(g.cam_kind) == 0 and int(f.cam_kind) != 0 and np.array_equal(g.cam[:12], np.asarray(f.cam)[:12]) and (g.cam[12:] == 0).all()
        assert g.prim_geom is f.prim_geom
