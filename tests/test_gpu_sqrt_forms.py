"""The fp32 square root's short forms (csrc/rt_device.hpp, round 11) against the correctly rounded library sqrtf of
the same build, compared on the device (tests/device/rt_devforms.hip):

* sqrt_nd over every bit pattern of its contract -- +-0, |x| >= 2^-96, +-inf, every NaN -- in one launch;
* sqrt_rg (v_rsq_f32, one multiply, one residual step: what sqrt_len's ballot lets through) over [2^-96, +inf);
* sqrt_len in single waves where one lane holds a tiny nonzero argument of either sign, a zero or +inf, so the
  ballot sends the other 63 lanes through the library's sequence.

The bar is 0 mismatches, two NaNs counting as equal.  That sqrtf itself is the correctly rounded root on the inputs
these tests name is tests/test_sqrt_forms_cases.py's business (numpy's float32 sqrt against a float64 sqrt rounded
once, on the CPU), and the last test here ties the device's sqrtf to numpy's on those same inputs.
"""
import numpy as np
import pytest

import devforms_bind as df
import sqrt_forms_cases as sc
from device_math_cases import assert_bits, ref_sqrt

pytestmark = pytest.mark.gpu

F32 = np.float32
LO = int(F32(2.0 ** -96).view(np.uint32))      # 0x0F800000
INF = 0x7F800000


def test_sqrt_nd_every_bit_pattern_of_its_contract():
    mis, first, skipped = df.sqrt_forms_sweep(df.SQRT_ND)
    assert skipped == 2 * (LO - 1)              # the tiny nonzero arguments of either sign, and nothing else
    assert mis == 0, [hex(b) for b in first]


def test_sqrt_rg_every_bit_pattern_of_its_range():
    mis, first, skipped = df.sqrt_forms_sweep(df.SQRT_RG)
    assert (1 << 32) - skipped == INF - LO       # 2^-96 <= x < +inf
    assert mis == 0, [hex(b) for b in first]


def test_sqrt_len_one_odd_lane_per_wave():
    """Wave w holds 63 in-range arguments and, in lane w % 64, one argument the short form is not for."""
    x, odd = sc.mixed_waves()
    assert odd.reshape(-1, df.WAVE).sum(axis=1).tolist() == [1] * (x.size // df.WAVE)
    got, want = df.sqrt_len_map(x)
    assert_bits(got, want, "sqrt_len, one out-of-range lane per wave", [x])
    assert_bits(want, ref_sqrt(x), "device sqrtf vs numpy", [x])
    # the same waves with the odd lane put in range: every wave takes the short form
    y = np.where(odd, F32(2.0), x)
    got, want = df.sqrt_len_map(y)
    assert_bits(got, want, "sqrt_len, every lane in range", [y])


def test_device_sqrtf_is_numpys_on_the_named_cases():
    x = sc.cases()
    got, want = df.sqrt_len_map(x)
    assert_bits(want, ref_sqrt(x), "device sqrtf vs numpy", [x])
    assert_bits(got, want, "sqrt_len on the named cases", [x])
