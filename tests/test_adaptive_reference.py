"""The inputs of test_gpu_adaptive.py's oracle cases, judged on the CPU oracle alone: adaptive_reference.CASES are fit to test with.

For every case the retirement schedule is recomputed from the oracle's individual samples (nothing below is a recorded value) and three
conditions are asserted -- conditions on the inputs, not tolerances:

  * at least three distinct levels of n_t occur, each in at least 3 tiles: a frame that mixes sample counts, so a resolve that read one k for
    the whole frame, or a fold that wrote to the wrong state slot after the first compaction, cannot pass;
  * at least one tile is still active at the cap: the run ends by the cap, with a compacted list that was traced in every round;
  * no per-tile maximum of the noise plane, of any tile at any round, lies within relative 1e-6 of eps.  The device decides with Welford's M2
    as numpy does here; the two-pass formula over the same samples agrees with Welford on those maxima to about 1e-15 relative (below 1e-9 is
    asserted), so the device's decision cannot differ from this file's by rounding.

Measured when the cases were chosen (tiles per n_t; tiles still active at the cap; the nearest per-tile maximum to eps, relative):

  spheres 61x37  f64 / f32  16 / 16 / 64  eps 0.2    16: 5, 32: 5, 48: 5, 64: 25                              19 of 40    0.6 %
  mixed   61x37  f64        16 / 16 / 64  eps 0.5    16: 8, 32: 16, 48: 4, 64: 12                             8 of 40     0.3 %
  spheres 203x99 f64        8 / 8 / 48    eps 0.15   8: 6, 16: 24, 24: 109, 32: 31, 40: 23, 48: 145           134 of 338  0.24 %

If a case stops meeting a condition (a scene of frame_reference.py was edited), choose another eps; do not loosen the condition."""
import numpy as np
import pytest

import adaptive_reference as ar
import frame_reference as fr


def _oracle(request, precision):
    return request.getfixturevalue("oracle" if precision == "f64" else "oracle_f32")


@pytest.mark.parametrize("case", ar.CASES, ids=ar.case_id)
def test_case_is_fit_to_test_with(request, case):
    name, precision, (nx, ny), first, chunk, cap, eps = case
    o = _oracle(request, precision)
    smp, nseg, rounds = ar.reference_run(o, case)
    k, n_t, active, _ = rounds[-1]
    assert k == cap
    levels, counts = np.unique(n_t, return_counts=True)
    print(ar.case_id(case), dict(zip(levels.tolist(), counts.tolist())), "active %d of %d" % (active.sum(), active.size))
    assert (counts >= 3).sum() >= 3, dict(zip(levels.tolist(), counts.tolist()))
    assert active.sum() >= 1
    assert set(levels.tolist()) <= set(ar.rounds_of(first, chunk, cap))
    nearest = min(float(np.abs(worst[np.isfinite(worst)] / eps - 1.0).min()) for _, _, _, worst in rounds)
    print("nearest per-tile maximum to eps: %.3g relative" % nearest)
    assert nearest > 1e-6
    # Welford (what the device keeps) against the two-pass formula over the same samples
    m2 = ar.welford_m2(smp, [k for k, _, _, _ in rounds])
    # on the values the decisions are taken on, the per-tile maxima; 1e-9 is a thousandth of the margin asserted above
    gap = 0.0
    for k, _, _, _ in rounds:
        a, b = ar.tile_max(ar.stderr_plane(m2[k], k)), ar.tile_max(fr.stderr_two_pass(smp, k))
        sel = b > 0
        assert (a[~sel] == 0).all(), k
        gap = max(gap, float(np.abs(a[sel] / b[sel] - 1.0).max()))
    print("Welford against two-pass, per-tile maxima: %.3g relative" % gap)
    assert gap < 1e-9


@pytest.mark.parametrize("case", ar.CASES[:1], ids=ar.case_id)
def test_composed_frame_and_rays(request, case):
    """the composition helpers: a uniform n_t gives the in-order frame and the oracle's ray count, a mixed one takes every pixel from its level"""
    name, precision, (nx, ny), first, chunk, cap, eps = case
    o = _oracle(request, precision)
    smp, nseg, rounds = ar.reference_run(o, case)
    uniform = np.full((ny, nx), 13)
    lin, _, cnt = o.render(fr.scene(name, nx, ny), nx, ny, 13, fr.DEPTH, fr.SEED, nthreads=16)
    assert np.array_equal(ar.expected_frame(smp, uniform), lin) and ar.expected_rays(nseg, uniform) == int(cnt[0])
    n_px = ar.per_pixel(rounds[-1][1], nx, ny)
    frame = ar.expected_frame(smp, n_px)
    for n in np.unique(n_px):
        assert np.array_equal(frame[n_px == n], fr.frame_in_order(smp, int(n))[n_px == n])
    assert ar.expected_rays(nseg, n_px) < int(np.transpose(nseg, (1, 0, 2)).sum())


def test_schedule_rules():
    """the schedule on hand-made noise planes: retirement is permanent, a NaN keeps a tile, k = 1 retires nothing, eps = 0 retires equal samples"""
    nx, ny = 16, 8  # two tiles
    planes = {1: np.full((ny, nx), np.inf), 2: np.zeros((ny, nx)), 3: np.ones((ny, nx))}
    planes[2][:, 8:] = np.nan
    planes[3][:, :8] = 5.0  # the retired tile's noise "rises" again: it stays retired
    rounds = ar.schedule(lambda k: planes[k], nx, ny, 1, 1, 3, 1.0)
    assert [k for k, _, _, _ in rounds] == [1, 2, 3]
    assert rounds[0][2].all() and rounds[1][2].tolist() == [[False, True]] and not rounds[2][2].any()
    assert rounds[2][1].tolist() == [[2, 3]]
    assert ar.rounds_of(16, 16, 64) == [16, 32, 48, 64] and ar.rounds_of(5, 4, 12) == [5, 9, 12]
    rounds = ar.schedule(lambda k: np.zeros((ny, nx)), nx, ny, 2, 2, 8, 0.0)
    assert len(rounds) == 1 and not rounds[0][2].any()
