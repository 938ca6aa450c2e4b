"""The float32 Adam oracle's bias-correction powers (oracle/mlp.py:adam_beta_power, adam_alpha) against exact rational arithmetic.

The update kernels are promised bit for bit against this oracle (csrc/adam.h), so the oracle itself has to be the same on every host:
beta^t is the exact power of float32(beta) rounded ONCE to float32 -- what a correctly rounded powf gives, and the value the device's
`(float)pow((double)beta, (double)t)` aims at (whether it reaches it at every t is for the GPU tests of the update kernels to show).
numpy's float32 power is 1 ulp off for about one step count in seven, first at t = 4."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import mlp as omlp

F = np.float32
STEPS = list(range(1, 3001)) + [10**4, 5 * 10**4, 99999, 10**5]
# beta2^t: a float32 subnormal from t = 87 294 (below 2^-126), zero past t = 103 921 (below 2^-150); beta1^t: 829 and 987, inside 1..3000
B2_TAIL = [87000, 87293, 87294, 87295, 95000, 103000, 103920, 103921, 103922, 104000, 110000]


def _is_nearest_f32(c, x):
    """c (a float32) is the exact rational x rounded to the nearest float32, ties to even: c is no farther from x than either of its
    float32 neighbours, compared exactly. x's denominator is a power of two, as every float32's is (at most 2^149): the three
    distances are compared as integers over one common denominator."""
    c = F(c)
    dx = x.denominator.bit_length() - 1
    assert x.denominator == 1 << dx
    D = max(dx, 149)
    xn = x.numerator << (D - dx)

    def dist(y):
        fy = Fraction(float(y))
        return abs(xn - (fy.numerator << (D - (fy.denominator.bit_length() - 1))))

    d0 = dist(c)
    even = (int(np.array(c).view(np.uint32)) & 1) == 0
    return all(d0 < d or (d0 == d and even) for d in (dist(np.nextafter(c, F(-np.inf))), dist(np.nextafter(c, F(np.inf)))))


EXACT_MAX_T = 110000  # (the exact power of a later t is not formed: 24 bits per step)


def _power_is_nearest_f32(c, b, t):
    """c is b^t rounded to the nearest float32. Past EXACT_MAX_T: 0 < b < 1, so b^t <= b^EXACT_MAX_T, and when that is below half the
    smallest subnormal (2^-150, compared exactly) the nearest float32 of b^t is zero."""
    if t <= EXACT_MAX_T:
        return _is_nearest_f32(c, b ** t)
    assert 0 < b < 1 and b ** EXACT_MAX_T < Fraction(1, 2**150)
    return F(c) == 0 and not np.signbit(F(c))


@pytest.mark.parametrize("beta", [omlp.ADAM_B1, omlp.ADAM_B2])
def test_beta_power_is_the_exact_power_rounded_once(beta):
    b = Fraction(float(F(beta)))  # the float32 beta, exactly
    bad = [t for t in STEPS + [10**6] + (B2_TAIL if beta == omlp.ADAM_B2 else [])
           if not _power_is_nearest_f32(omlp.adam_beta_power(beta, t), b, t)]
    assert not bad, (beta, bad[:10], len(bad))


def test_beta_power_subnormal_and_zero_regions():
    tiny, denorm = F(np.finfo(np.float32).tiny), np.nextafter(F(0), F(1))
    for beta, first_sub, last_nonzero in ((omlp.ADAM_B1, 829, 986), (omlp.ADAM_B2, 87294, 103921)):
        p = lambda t: omlp.adam_beta_power(beta, t)
        assert p(first_sub - 1) >= tiny > p(first_sub) > 0  # the first subnormal
        assert p(last_nonzero) == denorm and p(last_nonzero + 1) == 0  # the last non-zero value is the smallest subnormal
        assert all(type(p(t)) is np.float32 for t in (1, first_sub, last_nonzero + 1))
    # far past the sampled exact range: beta < 1, so beta^t <= beta^110000 < 2^-150 (shown exactly above) and the power is zero
    for t in (10**6, 10**7, 2**31 - 1):
        assert omlp.adam_beta_power(omlp.ADAM_B1, t) == 0 and omlp.adam_beta_power(omlp.ADAM_B2, t) == 0
    assert Fraction(float(F(omlp.ADAM_B2))) ** 110000 < Fraction(1, 2**150)


def test_beta_power_never_rises_with_t():
    """Rounding once is monotone: beta^(t+1) <= beta^t in float32 (a power that is 1 ulp high at one t and exact at the next need not be)."""
    ts = STEPS + B2_TAIL + [10**6]
    for beta in (omlp.ADAM_B1, omlp.ADAM_B2):
        p = np.array([omlp.adam_beta_power(beta, t) for t in sorted(ts)])
        assert np.all(np.diff(p) <= 0) and p[0] == F(beta) and p[-1] == 0


@pytest.mark.parametrize("lr", [1e-3, 1e-4, 5e-5])
def test_adam_alpha_finite_positive_and_monotone_where_it_must_be(lr):
    ts = sorted(STEPS + B2_TAIL + [10**6])
    a = np.array([omlp.adam_alpha(lr, t) for t in ts])
    assert a.dtype == np.float32 and np.all(np.isfinite(a)) and np.all(a > 0)
    assert a[0] == F(F(lr) * np.sqrt(F(1) - F(omlp.ADAM_B2)) / (F(1) - F(omlp.ADAM_B1)))  # t = 1: the betas themselves
    # from t = 165 on beta1^t < 2^-25 and 1 - beta1^t is 1: alpha = lr sqrt(1 - beta2^t), a chain of monotone roundings of a value
    # that rises with t
    late = np.array([x for t, x in zip(ts, a) if t >= 165])
    assert F(1) - omlp.adam_beta_power(omlp.ADAM_B1, 165) == 1 and np.all(np.diff(late) >= 0)
    # from beta2^t < 2^-25 (t = 17 321) on it is the step size itself
    assert F(1) - omlp.adam_beta_power(omlp.ADAM_B2, 17321) == 1
    assert all(x == F(lr) for t, x in zip(ts, a) if t >= 17321) and a[-1] == F(lr)
    assert np.all(a <= F(lr))  # the bias correction never enlarges the step (sqrt(1 - b2^t) <= 1 - b1^t for these betas)


def test_float64_path_is_unchanged():
    for t in (1, 4, 9, 1000):
        assert omlp.adam_beta_power(omlp.ADAM_B1, t, np.float64) == np.power(np.float64(omlp.ADAM_B1), np.float64(t))
        want = np.float64(1e-3) * np.sqrt(1 - np.power(np.float64(omlp.ADAM_B2), np.float64(t))) / (1 - np.power(np.float64(omlp.ADAM_B1), np.float64(t)))
        assert omlp.adam_alpha(1e-3, t, np.float64) == want and type(omlp.adam_alpha(1e-3, t, np.float64)) is np.float64


def test_regression_first_step_counts_numpy_float32_power_misses():
    """beta1^4 = 0.65609993047... -> 0x3f27f62a (numpy's float32 power gives 0x3f27f62b, printed 0.6561); beta2^9 = 0.99103603107...
    -> 0x3f7db48a (numpy: 0x3f7db489). The first step counts at which the oracle's former form was not the correctly rounded value."""
    bits = lambda x: int(np.array(F(x)).view(np.uint32))
    assert bits(omlp.adam_beta_power(omlp.ADAM_B1, 4)) == 0x3F27F62A
    assert bits(omlp.adam_beta_power(omlp.ADAM_B2, 9)) == 0x3F7DB48A
    # the step sizes they give (with numpy's float32 powers: 0x3940b1a1, 0x3922108f at lr = 1e-3; 0x379a27b3, 0x3781a6d9 at 1e-4)
    assert [bits(omlp.adam_alpha(1e-3, t)) for t in (4, 9)] == [0x3940B19F, 0x3922106B]
    assert [bits(omlp.adam_alpha(1e-4, t)) for t in (4, 9)] == [0x379A27B1, 0x3781A6BC]
    assert _is_nearest_f32(np.array(0x3F27F62A, np.uint32).view(np.float32), Fraction(float(F(0.9))) ** 4)
    assert not _is_nearest_f32(np.array(0x3F27F62B, np.uint32).view(np.float32), Fraction(float(F(0.9))) ** 4)
