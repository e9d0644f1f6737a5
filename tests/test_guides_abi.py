"""rt_render_guides_async and GpuRenderer.guides: what can be checked without a GPU.  The entry point checks its
pointers before any HIP call, so a NULL argument is refused on a machine without a device; the renderer checks
its mode and the output names before it touches its context; and the reduction the GPU tests restate is checked
here against a literal 64-slot loop."""
import ctypes
import re

import numpy as np
import pytest

import rt_mi355x as rt
from rt_mi355x import abi
from rt_mi355x import renderer as rmod
from guide_restatement import fold   # the GPU tests' restatement


def test_symbol_is_exported_and_declared():
    assert "rt_render_guides_async" in abi.EXPORTED
    text = open(abi.SOURCE_FILES[-1]).read()
    assert "int rt_render_guides_async(" in text
    # the header states the definition: the reduction order and the premultiplied means
    assert "s % 64 == j" in text and "p[i] += p[i + h]" in text and "premultiplied by coverage" in text
    assert "rt_guides.hpp" in abi.KERNEL_SOURCES


def test_null_arguments_are_refused_without_a_gpu(lib):
    cam = rt.camera_new_py(4, 3, **rt.MAIN_CAMERA)
    out = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    calls = [
        (None, ctypes.byref(cam), 4, 1, 0, None, out, out, out, out, None),      # NULL ctx
        (ctx, None, 4, 1, 0, None, out, out, out, out, None),                    # NULL camera
        (ctx, ctypes.byref(cam), 4, 1, 0, None, None, None, None, None, None),   # all four outputs NULL
        (ctx, ctypes.byref(cam), 0, 1, 0, None, out, out, out, out, None),       # spp == 0
    ]
    for args in calls:
        assert lib.rt_render_guides_async(*args) == abi.RT_ERR_INVALID
        assert b"rt_render_guides_async" in lib.rt_last_error(), lib.rt_last_error()


def test_kernel_guides_bit_decodes_alike_in_c_and_python():
    text = open(abi.SOURCE_FILES[-1]).read()
    m = re.search(r"#define RT_KERNEL_GUIDES\(id\) \(\(\(id\) >> (\d+)\) & 1u\)", text)
    assert m and int(m.group(1)) == 11
    for kid in (0x8000 | 1 << 11, 0x8000 | 1 << 11 | 1 | 4 << 1 | 1 << 7, 0x8000 | 1 << 11 | 5 << 1 | 1 << 8,
                0x808C, 0x81F9, 0x8000 | 1 << 9 | 1 << 10):
        k = abi.kernel_info(kid)
        assert abi.RT_KERNEL_GUIDES(kid) == (kid >> int(m.group(1))) & 1
        assert k["guides"] == bool(abi.RT_KERNEL_GUIDES(kid))
    assert abi.kernel_name(0x8000 | 1 << 11 | 1 | 4 << 1 | 1 << 7) == "guide_pixels<double,true,false>"
    assert abi.kernel_name(0x8000 | 1 << 11 | 5 << 1 | 1 << 8) == "guide_pixels<float,false,true>"
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"   # unchanged


class NoGpu(rmod.GpuRenderer):   # any use of the context would raise AttributeError, not ValueError
    def __init__(self, flags):
        self.flags = flags

    def __del__(self):
        pass


@pytest.mark.parametrize("flags", [abi.RT_FLAG_ROOT2, abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2, abi.RT_FLAG_MODE_VECTORIZED,
                                   abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_F32 | abi.RT_FLAG_MODE_VECTORIZED3])
def test_guides_refuses_other_modes_before_any_gpu_call(flags):
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).guides(4, None, None)
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).guides_flat(4, None, None)


def test_guides_flat_refuses_unknown_names_before_any_gpu_call():
    with pytest.raises(ValueError, match="unknown guide buffer"):
        NoGpu(abi.RT_FLAG_F32).guides_flat(4, None, None, want=("albedo", "colour"))
    assert rmod.GUIDE_NAMES == ("albedo", "normal", "depth", "coverage")
    assert rt.Guides._fields == rmod.GUIDE_NAMES


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_fold_is_the_literal_64_slot_reduction(n):
    vals = np.random.default_rng(n).standard_normal(n) * 10.0 ** np.random.default_rng(n + 1).integers(-3, 4, n)
    slots = [0.0] * 64
    for s in range(n):
        slots[s % 64] = slots[s % 64] + float(vals[s])
    for h in (32, 16, 8, 4, 2, 1):
        for i in range(h):
            slots[i] = slots[i] + slots[i + h]
    want = np.float32(slots[0] / float(n))
    got = fold(vals)
    assert got.dtype == np.float32 and got == want
    # n ones sum to n: the constants a sky pixel writes without tracing are the definition's
    assert fold(np.ones(n)) == np.float32(1.0) and fold(np.zeros(n)) == np.float32(0.0)
