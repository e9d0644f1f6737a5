"""CPU companion of tests/test_gpu_sqrt_forms.py: the reference the GPU test compares with is itself the correctly
rounded root on the inputs the GPU test names.  numpy's float32 sqrt must agree, bit for bit, with the float64 sqrt
rounded once to float32 (the float64 sqrt is correctly rounded and 53 >= 2 * 24 + 2, so rounding it again is harmless),
and the generated inputs must be what their docstrings say."""
import numpy as np

import sqrt_forms_cases as sc
from device_math_cases import assert_bits, ref_sqrt, ref_sqrt_via_f64

F32, U32 = np.float32, np.uint32


def test_numpy_sqrt_is_the_f64_sqrt_rounded_once_on_the_named_cases():
    x = sc.cases()
    assert x.dtype == F32 and x.size == 1 << 20
    assert_bits(ref_sqrt(x), ref_sqrt_via_f64(x), "numpy float32 sqrt vs float64 sqrt rounded", [x])


def test_named_cases_hold_what_they_name():
    x = sc.cases()
    b = set(x.view(U32).tolist())
    for e in range(sc.LO >> 23, 255):                       # every binade from 2^-96: its first and last patterns
        assert {e << 23, (e << 23) + 1} <= b
        assert {(e << 23) - 1, (e << 23) - 2} <= b or e == sc.LO >> 23
    assert {sc.LO, 0x00000000, 0x80000000, sc.INF, 0x7FC00000} <= b
    # exact squares with both neighbours: the root is exact, the neighbours' roots round to it or next to it
    r = ref_sqrt(x)
    with np.errstate(all="ignore"):                          # the NaN and inf cases
        exact = (r.astype(np.float64) ** 2 == x.astype(np.float64)) & sc.in_range(x) & (x.view(U32) > sc.LO)
    assert exact.sum() >= 150000
    sq = x.view(U32)[exact][:1000]
    assert all({int(s) - 1, int(s) + 1} <= b for s in sq)
    assert sc.in_range(x).mean() > 0.99


def test_mixed_waves_hold_one_odd_lane_each():
    x, odd = sc.mixed_waves()
    assert x.size % 256 == 0 and x.size == sc.ODD.size * 64 * 64
    ok = sc.in_range(x)
    assert (ok == ~odd).all()                               # the odd lane, and it alone, is out of range
    lanes = np.argwhere(odd.reshape(-1, 64))[:, 1].reshape(sc.ODD.size, 64)
    assert (lanes == np.arange(64)).all()                   # every kind visits every lane
    assert_bits(ref_sqrt(x), ref_sqrt_via_f64(x), "numpy float32 sqrt vs float64 sqrt rounded", [x])
