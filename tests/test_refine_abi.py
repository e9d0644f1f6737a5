"""rt_progressive_refine / rt_progressive_refine_items and GpuRenderer.adaptive(plan=...): what can be checked
without a GPU.  The entry points check their pointers before any HIP call, so a NULL argument is refused on a
machine without a device; the plan argument is checked before the renderer touches its context."""
import ctypes

import pytest

import rt_mi355x as rt
from rt_mi355x import abi
from rt_mi355x import renderer as rmod


def test_refine_symbols_refuse_null(lib):
    assert "rt_progressive_refine" in abi.EXPORTED and "rt_progressive_refine_items" in abi.EXPORTED
    na, ns, s = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7)
    calls = [
        (lib.rt_progressive_refine, (None, 0.5, 8, None, ctypes.byref(na), ctypes.byref(ns))),
        (lib.rt_progressive_refine, (None, 0.5, 8, None, None, None)),
        (lib.rt_progressive_refine_items, (None, ctypes.byref(s), ctypes.byref(na), None, 0)),
        (lib.rt_progressive_refine_items, (None, None, None, None, 0)),
    ]
    for fn, args in calls:
        assert fn(*args) == abi.RT_ERR_INVALID
        assert fn.__name__.encode() in lib.rt_last_error(), lib.rt_last_error()


def test_header_documents_the_readback():
    text = open(abi.SOURCE_FILES[-1]).read()
    assert "int rt_progressive_refine(" in text and "int rt_progressive_refine_items(" in text
    assert "no _async suffix" in text


def test_unknown_plan_is_refused_before_any_gpu_call():
    assert rt.renderer.check_adaptive(8, 64, 0.1) == (8, 64, 0.1)
    assert rt.renderer.check_adaptive(8, 64, 0.1, "device") == (8, 64, 0.1)
    with pytest.raises(ValueError, match="plan"):
        rt.renderer.check_adaptive(8, 64, 0.1, "gpu")

    class NoGpu(rmod.GpuRenderer):   # any use of the context would raise AttributeError, not ValueError
        def __init__(self):
            pass

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="plan"):
        NoGpu().adaptive(8, 8, 64, 0.1, None, None, plan="both")
