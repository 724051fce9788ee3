"""The lemma behind the one-numerator sphere test (rtmi_device.h: sphere_roots), checked on the CPU with numpy doing exactly the device's
operations, one IEEE rounding each: for a ray whose origin is inside or on the sphere (c <= 0) and whose a = d.d lies in [2^-200, 2^200), the
first root fl((-b - sq) / a), sq = sqrt(fl(fl(b b) - fl(a c))), never exceeds 2^-300 -- the smallest t-min under which the selector is on -- so
`t > t-min` fails and the lane may form the second root directly.  In the zone where b b underflows the numerator itself can be positive:
that is why the selector asks for the certified ranges and not for c <= 0 alone."""
from fractions import Fraction

import numpy as np

N = 4_000_000
T_MIN_FLOOR = 2.0 ** -300


def _pow2(rng, n, lo, hi):
    """n doubles m 2^e, m in [1, 2), e uniform in [lo, hi)"""
    return np.ldexp(1.0 + rng.random(n), rng.integers(lo, hi, n).astype(np.int32))


def _operands(seed, b_lo, b_hi):
    rng = np.random.default_rng(seed)
    b = _pow2(rng, N, b_lo, b_hi) * rng.choice([-1.0, 1.0], N)
    c = -_pow2(rng, N, -700, 700)
    c[rng.random(N) < 0.05] = -0.0
    c[rng.random(N) < 0.05] = 0.0
    a = _pow2(rng, N, -200, 200)
    return b, c, a


def _first_root(b, c, a):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        disc = b * b - a * c
        sq = np.sqrt(disc)
        n1 = -b - sq
        return disc, n1, n1 / a


def test_first_root_never_passes_t_min_from_inside():
    b, c, a = _operands(1, -480, 530)  # up to where b b overflows
    disc, n1, t = _first_root(b, c, a)
    assert (disc >= 0).all()  # every one of these lanes reaches the roots
    assert not (t > T_MIN_FLOOR).any(), int((t > T_MIN_FLOOR).sum())
    assert not (n1 > 0).any(), "outside the underflow zone the numerator itself is <= 0 (or -inf / NaN where b b overflows)"
    with np.errstate(over="ignore"):
        over = np.isinf(b * b)
    assert over.any() and (np.isneginf(n1[over]) | np.isnan(n1[over])).all()


def test_underflow_zone_needs_the_certified_ranges():
    b, c, a = _operands(2, -1074, -480)
    disc, n1, t = _first_root(b, c, a)
    assert (disc >= 0).all()
    assert not (t > T_MIN_FLOOR).any(), int((t > T_MIN_FLOOR).sum())
    positive = int((n1 > 0).sum())
    print("numerators above 0 in the underflow zone:", positive, "of", N)
    assert positive > 0, "c <= 0 alone does not make the numerator <= 0 here"
    assert (n1[n1 > 0] < 2.0 ** -480).all()


def _fma(x, y, z):
    return float(Fraction(x) * Fraction(y) + Fraction(z))  # exact, then one correct rounding (int / int)


def test_per_ray_reciprocal_form_of_the_first_root():
    """the quotient a `fast` lane really forms, q = fl(n r), t = fma(fma(-a, q, n), r, q), on a sample of both zones (r = RN(1 / a) stands in for the
    refined reciprocal): never above 2^-300 either"""
    for seed, lo, hi in ((3, -480, 511), (4, -1074, -480)):
        b, c, a = _operands(seed, lo, hi)
        disc, n1, _ = _first_root(b[:4000], c[:4000], a[:4000])
        for n, av in zip(n1.tolist(), a[:4000].tolist()):
            r = 1.0 / av
            q = n * r
            t = _fma(_fma(-av, q, n), r, q)
            assert not t > T_MIN_FLOOR, (n, av, t)


def test_second_root_is_monotone_behind_the_first():
    """the second-root arm is entered on `!(t > t-min)` alone: a first root that failed `t < best` is followed by a second one that is no smaller"""
    rng = np.random.default_rng(5)
    b = _pow2(rng, N, -60, 60) * rng.choice([-1.0, 1.0], N)
    sq = _pow2(rng, N, -60, 60)
    sq[rng.random(N) < 0.05] = 0.0
    a = _pow2(rng, N, -200, 200)
    assert ((-b + sq) / a >= (-b - sq) / a).all()
