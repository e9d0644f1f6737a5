"""ctypes binding of the short-form probes of the test-only device library (tests/device/rt_devforms.hip, built
into rust-ray-tracing_amd/lib/librt_devunit.so): sqrt_rg / sqrt_nd / sqrt_len of csrc/rt_device.hpp against the
library sqrtf of the same build, compared on the device.

The sweep takes no input: one launch covers all 2^32 bit patterns.  The map takes whole waves the caller arranged:
n is a multiple of 256 and lane i of the launch holds entry i, so a wave is x[64 w : 64 w + 64].
"""
import ctypes

import numpy as np

import devunit_bind as du

WAVE = du.WAVE
BLOCK = du.BLOCK
SQRT_ND, SQRT_RG = 0, 1

_bound = False


def _lib():
    global _bound
    lib = du.load_devunit()
    if not _bound:
        vp, sz, u64p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
        lib.du_sqrt_forms_sweep.argtypes, lib.du_sqrt_forms_sweep.restype = [ctypes.c_int, u64p, u64p, vp], ctypes.c_int
        lib.du_sqrt_len_map.argtypes, lib.du_sqrt_len_map.restype = [vp, vp, vp, sz], ctypes.c_int
        _bound = True
    return lib


def sqrt_forms_sweep(which):
    """SQRT_ND: sqrt_nd over every pattern of its contract (all but the tiny nonzero ones of either sign); SQRT_RG:
    sqrt_rg over [2^-96, +inf).  Returns (mismatches against sqrtf, the first up to 8 offending bit patterns,
    patterns outside the contract and so not tested)."""
    mis, skipped = ctypes.c_uint64(0), ctypes.c_uint64(0)
    first = np.zeros(8, np.uint32)
    rc = _lib().du_sqrt_forms_sweep(which, ctypes.byref(mis), ctypes.byref(skipped), first.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"du_sqrt_forms_sweep: HIP error {rc}")
    return mis.value, first[:min(mis.value, 8)], skipped.value


def sqrt_len_map(x):
    """(sqrt_len(x), sqrtf(x)) per lane, both from the device."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 1 and x.size and x.size % BLOCK == 0, x.shape
    got, want = np.empty_like(x), np.empty_like(x)
    rc = _lib().du_sqrt_len_map(x.ctypes.data, got.ctypes.data, want.ctypes.data, x.size)
    if rc != 0:
        raise RuntimeError(f"du_sqrt_len_map: HIP error {rc}")
    return got, want
