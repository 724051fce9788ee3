"""CPU self-checks of denoise_reference.py, the numpy restatement the GPU tests pin the filter kernel against: the restatement must itself be
the filter include/rtmi.h describes -- identity at 0 passes, the plain B3 a-trous blur when no edge term is on, edges the features mark are
kept, and the stated behaviour at se = +inf, NaN and inf pixels."""
import numpy as np

import denoise_reference as dr
import frame_reference as fr

NX, NY = 61, 37


def test_zero_iterations_is_the_identity():
    lin, se, ft = dr.synthetic_frame(NX, NY)
    lin[3, 4] = np.nan
    se[5, 6] = np.inf
    out, q, err = dr.denoise(lin, se, ft, iterations=0, sigma_c=2.0, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)
    assert np.array_equal(out, lin, equal_nan=True) and np.array_equal(err, se)
    assert np.array_equal(q, fr.quantise(lin))
    out, _, err = dr.denoise(lin, None, None, iterations=0)
    assert np.array_equal(out, lin, equal_nan=True) and not err.any()


def test_without_edge_terms_a_pass_is_the_b3_blur_with_border_renormalisation():
    """every sigma 0: x = 0, r = 1, w = h[dy] h[dx] exactly, so a pass is sum(w c) / sum(w) over the taps inside the image.  The separable form
    adds the same 25 products in another order: each side rounds at most 25 additions, one product per term and a division, all of
    non-negative terms, so the two differ by less than 2 * 30 * 2^-53 relative: 1e-14."""
    lin, se, ft = dr.synthetic_frame(NX, NY, seed=3)
    lin = np.abs(lin)
    for have_se, have_ft in ((True, True), (False, False)):
        out, _, err = dr.denoise(lin, se if have_se else None, ft if have_ft else None, iterations=1)
        assert np.allclose(out, dr.b3_blur(lin), rtol=1e-14, atol=0)
    # the variance of the mean: sum(w^2 V) / sum(w)^2 -- a weighted mean of independent pixels
    out, _, err = dr.denoise(lin, se, None, iterations=1)
    w = np.outer(dr.B3, dr.B3)
    y, x = 20, 30
    exp = (w ** 2 * (se[y - 2:y + 3, x - 2:x + 3] ** 2)).sum() / w.sum() ** 2
    assert np.isclose(err[y, x] ** 2, exp, rtol=1e-13)
    assert (err[2:-2, 2:-2] < se[2:-2, 2:-2].max()).all()
    # pass i uses step 2^i: a single bright pixel spreads to exactly the a-trous footprint
    spike = np.zeros((33, 33, 3))
    spike[16, 16] = 1.0
    two, _, _ = dr.denoise(spike, None, None, iterations=2)
    ys, xs = np.nonzero(two[..., 0])
    assert ys.min() == 16 - 6 and ys.max() == 16 + 6 and xs.min() == 16 - 6 and xs.max() == 16 + 6


def test_a_step_the_features_mark_survives_five_passes():
    rng = np.random.default_rng(5)
    lin = np.zeros((NY, NX, 3))
    lin[:, : NX // 2] = 0.2
    lin[:, NX // 2:] = 0.8
    noise = 0.02 * rng.normal(size=lin.shape)
    se = np.full((NY, NX), 0.02)
    ft = np.zeros((NY, NX, dr.FEATURES))
    ft[:, : NX // 2, 0:3] = (0.1, 0.5, 0.9)
    ft[:, NX // 2:, 0:3] = (0.9, 0.5, 0.1)
    ft[..., 5] = 1.0
    ft[..., 6] = 4.0
    ft[..., 7] = 1.0
    # the features alone: inside a side every weight is h[dy] h[dx] (equal features), across the step the albedo term gives
    # x = 1.28 / 0.01 and w < 4e-9 of a tap's weight: five passes average the noise away and leave the step where it is
    kept, _, err = dr.denoise(lin + noise, se, ft, iterations=5, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)
    blurred, _, _ = dr.denoise(lin + noise, se, ft, iterations=5)
    assert np.abs(kept - lin).max() < 0.02, "the step stands and the noise (sigma 0.02) has gone down on both sides"
    assert np.abs(kept - lin).std() < 0.25 * noise.std()
    assert np.abs(blurred - lin).max() > 0.2, "without edge terms five passes smear the step"
    assert err.max() < 0.02
    # with the colour term as well the step still stands (the colour term only ever lowers a weight), and the noise still goes down
    both, _, _ = dr.denoise(lin + noise, se, ft, iterations=5, sigma_c=2.0, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)
    assert np.abs(both - lin).std() < noise.std() and np.abs(both - lin).max() < np.abs(noise).max()
    # the colour term alone keeps a step that stands 30 standard errors above the noise estimate: the columns next to it keep their side's value
    alone, _, _ = dr.denoise(lin + noise, se, None, iterations=5, sigma_c=2.0)
    assert abs(alone[:, NX // 2 - 1].mean() - 0.2) < 0.01 and abs(alone[:, NX // 2].mean() - 0.8) < 0.01
    assert np.abs(alone - lin).std() < noise.std()


def test_infinite_stderr_nan_and_inf_pixels():
    lin, se, ft = dr.synthetic_frame(NX, NY, seed=7)
    se1 = se.copy()
    se1[10:14, 20:24] = np.inf  # one-sample pixels: no colour edge, they are filtered like their neighbours by the other terms
    out, _, err = dr.denoise(lin, se1, ft, iterations=3, sigma_c=2.0, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)
    assert np.isfinite(out).all() and not np.isnan(err).any()
    assert np.isinf(err[10:14, 20:24]).all(), "a variance of +inf stays +inf where it has weight"
    free, _, _ = dr.denoise(lin, se1, None, iterations=1, sigma_c=2.0)
    blur = dr.b3_blur(lin)
    assert np.allclose(free[12, 22], blur[12, 22], rtol=1e-13), "se = +inf: the colour term is 0, the pixel takes the plain blur"
    # NaN and inf colours: the pixel passes through, and no neighbour takes it as a tap
    bad = lin.copy()
    bad[5, 5] = np.nan
    bad[20, 40, 1] = np.inf
    bad[30, 10, 2] = -np.inf
    out, q, err = dr.denoise(bad, se, ft, iterations=5, sigma_c=2.0, sigma_n=0.3, sigma_a=0.1, sigma_d=0.1)
    for y, x in ((5, 5), (20, 40), (30, 10)):
        assert np.array_equal(out[y, x], bad[y, x], equal_nan=True) and err[y, x] == np.sqrt(se[y, x] * se[y, x])
    ok = np.isfinite(bad).all(axis=2)
    assert np.isfinite(out[ok]).all() and np.isfinite(err[ok]).all()
    assert np.array_equal(q, fr.quantise(out))
    # a NaN in the noise estimate: every weight that reads it is NaN, the tap is skipped; the pixel itself has no tap left and passes through
    se2 = se.copy()
    se2[8, 8] = np.nan
    out, _, err = dr.denoise(lin, se2, None, iterations=1, sigma_c=2.0)
    assert np.array_equal(out[8, 8], lin[8, 8]) and np.isnan(err[8, 8]) and np.isfinite(out).all()
    assert np.isfinite(np.delete(err.ravel(), 8 * NX + 8)).all()


def test_feature_fold_is_the_frames_fold():
    rng = np.random.default_rng(11)
    for R in (np.float64, np.float32):
        smp = rng.random((5, 4, 7, dr.FEATURES)).astype(R)
        img = dr.feature_frame(smp)
        acc = smp[:, :, 0]
        for s in range(1, 7):
            acc = acc + smp[:, :, s]
        exp = (acc * (R(1) / R(7))).astype(np.float64)
        assert img.shape == (4, 5, dr.FEATURES) and np.array_equal(img, np.transpose(exp, (1, 0, 2))[::-1])
        assert np.array_equal(dr.feature_frame(smp, 1), np.transpose(smp[:, :, 0].astype(np.float64), (1, 0, 2))[::-1])
