"""The inputs of test_gpu_frame_exact.py, judged on the CPU oracle alone: they can tell a wrong fold from the right one.

For the pinhole scenes of frame_reference.py every sample of a frame is rebuilt from the oracle's probes and folded with numpy.  The in-order
fold times 1 / ns is oracle.render's frame bit for bit, f64 and f32, and the probes' segment counts sum to its ray counter: the reconstruction
is right.  The same samples folded in another way are not that frame.  Two conditions are asserted, floors on what the GPU tests can see, so that
a later edit of a scene cannot blunt them unnoticed:

  * at most 25 % of a frame's pixels have all samples equal (thin lens, whose samples cannot be rebuilt: at most 25 % of the pixels are the same
    in the ns = 1 and ns = 2 frames);
  * every wrong fold changes at least 25 % of the pixels at every ns in NS_FOLD, in every precision the scene runs in.

Measured (share of pixels; "restart n": a fold that starts over at a boundary between sample passes of n instead of carrying the sum):

  scene    size    prec ns  all equal  reversed pairwise  sum / ns  restart 2  restart 4
  spheres  61x37   f64   7    0.058     0.657    0.553    0.690     1.000      0.998
  spheres  61x37   f64  13    0.053     0.771    0.714    0.699     1.000      1.000
  spheres  61x37   f32   7    0.058     0.659    0.529    0.911     1.000      0.998
  spheres  61x37   f32  13    0.053     0.770    0.735    0.782     1.000      1.000
  spheres  203x99  f64   7    0.063     0.655    0.549    0.685     0.999      0.996
  spheres  203x99  f64  13    0.061     0.783    0.742    0.692     1.000      1.000
  spheres  203x99  f32   7    0.063     0.639    0.530    0.910     0.999      0.996
  spheres  203x99  f32  13    0.061     0.771    0.744    0.786     1.000      1.000
  mixed    61x37   f64   7    0.031     0.513    0.423    0.461     1.000      1.000
  mixed    61x37   f64  13    0.030     0.640    0.565    0.510     1.000      1.000
  mixed    117x93  f64   7    0.046     0.499    0.416    0.469     1.000      1.000
  mixed    117x93  f64  13    0.044     0.640    0.559    0.501     1.000      1.000
  spheres-lens, ns = 1 frame against ns = 2 frame, share of equal pixels: 61x37 0.161, 203x99 0.174 (f64 and f32 alike)

ns = 1 (no addition) and ns = 2 (one addition, which commutes) cannot show an order; the GPU module runs them once as the edges of the fold, the
conditions hold at NS_FOLD.  "0 + first" in place of "start from the first" differs only for a sample of -0.0, which no path returns (color
starts from 0 + 1 * emitted, rt_oracle.c): it shows as 0 % here and is not asserted."""
import numpy as np
import pytest

import frame_reference as fr

SIZES = [(name, p, size) for name, p in fr.CASES if name != "spheres-lens" for size in (fr.SIZE, fr.SIZE_PASSES[name])]


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_render_stream_restatement(request, precision):
    o = _oracle(request, precision)
    pix, smp = np.array([0, 1, 7, 2256, 20096, 2 ** 40 + 3]), np.array([0, 1, 6, 12, 255, 2 ** 33])
    keys = fr.sample_keys(fr.SEED, pix, smp)
    assert [int(k) for k in keys] == [o.sample_key(fr.SEED, int(p), int(s)) for p, s in zip(pix, smp)]
    for d in (0, 1, 2, 77):
        assert fr.draws(keys, d, precision).astype(np.float64).tolist() == [o.draw(int(k), d) for k in keys]


@pytest.mark.parametrize("name,precision,size", SIZES)
def test_numpy_fold_is_the_oracle_frame(request, name, precision, size):
    o = _oracle(request, precision)
    nx, ny = size
    for ns in fr.NS_EDGE + fr.NS_FOLD:
        smp, nseg = fr.samples(o, name, nx, ny, ns)
        lin, q, cnt = o.render(fr.scene(name, nx, ny), nx, ny, ns, fr.DEPTH, fr.SEED, nthreads=16)
        assert np.array_equal(fr.frame_in_order(smp), lin), ns
        assert nseg == int(cnt[0]) and int(cnt[1]) == nx * ny, ns
        if precision == "f64":  # (the f32 oracle quantises in float: no such identity is promised there)
            assert np.array_equal(fr.quantise(lin), q), ns


@pytest.mark.parametrize("name,precision,size", SIZES)
def test_wrong_folds_are_told_apart(request, name, precision, size):
    o = _oracle(request, precision)
    nx, ny = size
    for ns in fr.NS_FOLD:
        smp, _ = fr.samples(o, name, nx, ny, ns)
        ref = fr.frame_in_order(smp)
        shares = {"all equal": fr.share_all_equal(smp)}
        shares.update({k: fr.share_changed(fold(smp), ref) for k, fold in fr.WRONG_FOLDS.items()})
        print(name, precision, size, ns, " ".join("%s %.3f" % kv for kv in shares.items()))
        assert shares.pop("all equal") <= 0.25, (ns, "too many pixels whose samples are all equal")
        for k, share in shares.items():
            assert share >= 0.25, (ns, k, share)


@pytest.mark.parametrize("precision", fr.PRECISIONS["spheres-lens"])
def test_thin_lens_frames_vary(request, precision):
    o = _oracle(request, precision)
    for nx, ny in (fr.SIZE, fr.SIZE_PASSES["spheres-lens"]):
        f = fr.scene("spheres-lens", nx, ny)
        assert int(f.cam_kind) == 1 and f.cam[21] > 0 and f.cam[23] > f.cam[22]  # a real aperture, a shutter interval
        one, two = (o.render(f, nx, ny, ns, fr.DEPTH, fr.SEED, nthreads=16)[0] for ns in (1, 2))
        share = float((one == two).all(axis=2).mean())
        print("spheres-lens", precision, nx, ny, "%.3f" % share)
        assert share <= 0.25


def test_scenes_hold_what_they_claim():
    f = fr.scene("spheres", *fr.SIZE)
    assert set(f.prim_kind.tolist()) == {0, 2} and set(f.tex_kind.tolist()) == {0} and set(f.mat_kind.tolist()) == {0, 1, 3}
    f = fr.scene("mixed", *fr.SIZE)
    assert set(f.prim_kind.tolist()) == {0, 2, 3, 4, 5, 6}           # spheres, moving spheres, the three rectangles, triangles
    assert set(f.tex_kind.tolist()) == {0, 3, 4, 8}                  # constant, Perlin noise, Perlin turbulence, image map: no sin
    assert set(f.mat_kind.tolist()) == {0, 1, 3}                     # lambertian, metal, diffuse light: no pow, no log
    assert f.prim_flip.any() and len(f.xform_kind) and set(f.xform_kind.tolist()) == {0, 1}
    assert f.tex_param[f.tex_kind == 0, :3].max() >= 10              # radiance far above 1
    for nx, ny in [fr.SIZE] + list(fr.SIZE_PASSES.values()):
        assert nx % 8 and ny % 8


def test_quantiser_witnesses_agree(oracle):
    """the numpy quantiser against the oracle's own (rto_quantise) on everything the GPU module feeds the device"""
    rng = np.random.default_rng(7)
    m = np.concatenate([fr.chosen_means(), rng.random(60000) * 1.2])
    m = np.concatenate([m, np.zeros(-len(m) % 3)]).reshape(-1, 3)
    got = fr.quantise(m)
    exp = np.stack([oracle.quantise(row) for row in m])
    assert np.array_equal(got, exp)
    b = fr.bucket_borders()
    assert (np.diff(b) > 0).all() and fr.quantise(b).tolist() == list(range(1, 256))
    edge = {0.0: 0, -0.0: 0, 5e-324: 0, 1.0: 255, 1.5: 255, 1e300: 255, np.inf: 255, -np.inf: 0, -1.0: 0, np.nan: 0}
    assert fr.quantise(list(edge)).tolist() == list(edge.values())
    assert fr.quantise(np.nextafter(1.0, 0.0)) == 255 and fr.quantise((255 / 255.99) ** 2 * (1 - 1e-15)) == 254


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (8, 8), (9, 17), (61, 37)])
@pytest.mark.parametrize("world", [1, 3, 8])
def test_tile_dealing_written_twice(size, world):
    """the dealing from the pixel side (deal) and from the tile side (coded_tiles) give the same gathered buffer, padding included"""
    nx, ny = size
    tx, ty = fr.tiles_of(nx, ny)
    per = (tx * ty + world - 1) // world + 2
    g, frame = fr.coded_tiles(nx, ny, world, per)
    assert g.tobytes() == fr.deal(frame, world, per).tobytes()
    inside = ~np.isnan(g)
    assert inside.sum() == nx * ny * 3 and len(np.unique(g[inside])) == nx * ny * 3  # every element its own code


def test_standard_error_reference(oracle):
    smp, _ = fr.samples(oracle, "spheres", *fr.SIZE, 7)
    assert np.isinf(fr.stderr_two_pass(smp, 1)).all()
    se = fr.stderr_two_pass(smp, 7)
    equal = fr.to_image((smp == smp[:, :, :1]).all(axis=2).astype(np.float64)).all(axis=2)
    assert equal.any() and (se[equal] == 0).all() and (se[~equal] > 0).all()
    per_channel = fr.to_image(np.sqrt(smp.astype(np.float64).var(axis=2, ddof=1) / 7))  # numpy's own variance as a second witness
    assert np.allclose(se[~equal], per_channel.max(axis=2)[~equal], rtol=1e-12, atol=0)
