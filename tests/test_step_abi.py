"""rt_scatter_async, rt_path_step_async and GpuRenderer.scatter / scatter_into / path_step / path_step_into: what can be
checked without a GPU.  The entry points check their arguments before any HIP call, so every refusal below happens on
a machine without a device, and the renderer checks shapes, dtypes and modes before it touches its context
(tests/test_query_abi.py's manner)."""
import ast
import ctypes
import re
import traceback

import numpy as np
import pytest

from rt_mi355x import abi
from rt_mi355x import renderer as rmod
from rt_mi355x import step_checks as checks
from test_abi import declared_functions
from test_query_abi import Dev, FakeDevice, NoGpu

HEADER = abi.SOURCE_FILES[-1]
F32 = abi.RT_FLAG_F32


# ---------------------------------------------------------------- the header and the binding
def test_symbols_are_exported_and_declared(lib):
    assert "rt_scatter_async" in abi.EXPORTED and "rt_path_step_async" in abi.EXPORTED
    assert sorted(abi.EXPORTED) == declared_functions()
    assert hasattr(lib, "rt_scatter_async") and hasattr(lib, "rt_path_step_async")
    text = open(HEADER).read()
    assert ("int rt_scatter_async(rt_context* ctx, uint64_t n_rays, const void* d_origins, const double* origin,\n"
            "                     const void* d_directions, const void* d_index, const void* d_t,\n"
            "                     const void* d_pixel, const void* d_sample, uint32_t bounce, uint64_t seed, uint32_t flags,\n"
            "                     void* d_colour, void* d_out_origins, void* d_out_directions, void* stream);") in text
    assert ("int rt_path_step_async(rt_context* ctx, uint64_t n_rays, void* d_origins, void* d_directions, void* d_colour,\n"
            "                       const void* d_pixel, const void* d_sample, uint32_t bounce, uint64_t seed, uint32_t flags,\n"
            "                       void* d_status, void* d_index, void* d_t, void* d_normal, void* d_front, void* stream);") in text
    assert "rt_step.hpp" in abi.KERNEL_SOURCES
    src = abi.kernel_source_text()
    assert "void scatter_rays(" in src and "void path_step_rays(" in src
    assert len(lib.rt_scatter_async.argtypes) == 16 and len(lib.rt_path_step_async.argtypes) == 16
    makefile = open(abi.PKG_DIR + "/Makefile").read()
    assert "csrc/rt_step.hpp" in makefile   # tests/test_abi.py holds the hash's file order to the Makefile's


def test_header_states_the_definitions():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    i = text.index("path steps: the material stage")
    assert i > text.index("int rt_query_occluded_async(")
    doc = text[i:text.index("int rt_scatter_async(", i)]
    for phrase in ("PackedHitRecords::finalize", "front taken before the negation", "Material::get_hit_result",
                   "one draw from stream 2 at counter (d_sample[i], d_pixel[i], bounce)", "the fp32 fold included",
                   "NOT normalised", "d_colour[i] *= attenuation", "its outputs are its inputs bit for bit",
                   "No ray's values depend on another ray", "d_index[i] >= n_spheres or d_sample[i] >= 2^20",
                   "rt_context_collect returns RT_ERR_INVALID", "bounce > RT_MAX_BOUNCES_F32", "n_rays > 0x7FFFFFFF",
                   "n_rays == 0: RT_OK", "both output arrays NULL", "both or neither origin form",
                   "samples = the scattered rays, ray_segments = bounce_iters = 0", "RT_KERNEL_SCATTER(kernel_id) is set",
                   "what rt_query_hits_async followed by rt_scatter_async does", "zeroing its direction",
                   "RT_STEP_SCATTERED, RT_STEP_MISSED (not scattered) or RT_STEP_INVALID",
                   "no value depends on which were asked for", "Origins are per ray only",
                   "samples = ray_segments = the valid rays", "RT_KERNEL_STEP(kernel_id) is set",
                   "under RT_FLAG_MODE_VECTORIZED", "allowed while a progressive session is open"):
        assert phrase in doc, phrase
    for name, value in (("RT_STEP_MISSED", 0), ("RT_STEP_SCATTERED", 1), ("RT_STEP_INVALID", 255)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(abi, name) == value


def test_kernel_bits_decode_alike_in_c_and_python():
    text = open(HEADER).read()
    for macro, bit, fn, key in (("RT_KERNEL_SCATTER", 16, abi.RT_KERNEL_SCATTER, "scatter"),
                                ("RT_KERNEL_STEP", 17, abi.RT_KERNEL_STEP, "step")):
        m = re.search(rf"#define {macro}\(id\) \(\(\(id\) >> (\d+)\) & 1u\)", text)
        assert m and int(m.group(1)) == bit and bit > 15
        for kid in (0x8000 | 1 << bit, 0x8000 | 1 << bit | 1 | 4 << 1, 0x8000 | 1 << bit | 5 << 1 | 1 << 8 | 1 << 4, 0x808C,
                    0x81F9, 0x8000 | 1 << 12 | 1 << 7, 0x8000 | 1 << 13, 0x8000 | 1 << 14, 0x8000 | 1 << (33 - bit)):
            assert fn(kid) == (kid >> bit) & 1 and abi.kernel_info(kid)[key] == bool((kid >> bit) & 1)
    s, p = 0x8000 | 1 << 16, 0x8000 | 1 << 17
    assert abi.kernel_name(s) == "scatter_rays<float>" and abi.kernel_name(s | 1) == "scatter_rays<double>"
    assert abi.kernel_name(p | 1 | 4 << 1) == "path_step_rays<double,false,false>"
    assert abi.kernel_name(p | 5 << 1 | 1 << 8 | 1 << 4) == "path_step_rays<float,true,true>"
    assert abi.kernel_name(p | 5 << 1 | 1 << 8) == "path_step_rays<float,false,true>"
    # older ids decode unchanged
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"
    assert abi.kernel_name(0x81F9) == "trace_paths<double,4,true,3,true,true>"
    assert abi.kernel_name(0x8000 | 1 << 12 | 1 | 4 << 1 | 1 << 7) == "query_rays<double,false,true,false>"
    assert abi.kernel_name(0x8000 | 1 << 13 | 6 << 1) == "trace_paths_rays<float,6,false,false>"
    assert abi.kernel_name(0x8000 | 1 << 14 | 5 << 1 | 1 << 8) == "occlusion_rays<float,false,true>"
    assert abi.kernel_name(0x8000 | 1 << 11 | 1 | 4 << 1 | 1 << 7) == "guide_pixels<double,true,false>"
    assert abi.kernel_name(0x8000 | 1 << 9 | 1 << 10 | 5 << 1) == "trace_paths_items<float,5,false,false>"
    k = abi.kernel_info(0x808C)
    assert not k["scatter"] and not k["step"] and abi.kernel_info(0) is None
    # the launch code's bits are the header's
    launch = open([f for f in abi.SOURCE_FILES if f.endswith("rt_launch.hpp")][0]).read()
    assert "kKernelScatterBit = 1u << 16" in launch and "kKernelStepBit = 1u << 17" in launch


# ---------------------------------------------------------------- the entry points' refusals
def scatter(lib, ctx, n, d_org, origin, d_dir, d_idx, d_t, d_pix, d_smp, bounce, flags, d_col, d_oo, d_od):
    o3 = None if origin is None else (ctypes.c_double * 3)(*origin)
    return lib.rt_scatter_async(ctx, n, d_org, o3, d_dir, d_idx, d_t, d_pix, d_smp, bounce, 7, flags, d_col, d_oo, d_od, None)


def step(lib, ctx, n, d_org, d_dir, d_col, d_pix, d_smp, bounce, flags, outs):
    return lib.rt_path_step_async(ctx, n, d_org, d_dir, d_col, d_pix, d_smp, bounce, 7, flags, *outs, None)


def test_scatter_arguments_are_refused_without_a_gpu(lib):
    p = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    O = (1.0, 2.0, 3.0)
    invalid = [
        ("NULL ctx", (None, 64, p, None, p, p, p, p, p, 0, 0, p, p, p)),
        ("NULL directions", (ctx, 64, p, None, None, p, p, p, p, 0, 0, p, p, p)),
        ("NULL index", (ctx, 64, p, None, p, None, p, p, p, 0, 0, p, p, p)),
        ("NULL t", (ctx, 64, p, None, p, p, None, p, p, 0, 0, p, p, p)),
        ("NULL pixel", (ctx, 64, p, None, p, p, p, None, p, 0, 0, p, p, p)),
        ("NULL sample", (ctx, 64, p, None, p, p, p, p, None, 0, F32, p, p, p)),
        ("both outputs NULL", (ctx, 64, p, None, p, p, p, p, p, 0, 0, p, None, None)),
        ("both origin forms", (ctx, 64, p, O, p, p, p, p, p, 0, 0, p, p, p)),
        ("neither origin form", (ctx, 64, None, None, p, p, p, p, p, 0, 0, None, p, p)),
        ("unknown flag bits", (ctx, 64, p, None, p, p, p, p, p, 0, 0x20, p, p, p)),
        ("unknown flag bits with F32", (ctx, 64, None, O, p, p, p, p, p, 0, F32 | 0x100, p, None, p)),
    ]
    for what, args in invalid:
        assert scatter(lib, *args) == abi.RT_ERR_INVALID, what
        assert b"rt_scatter_async" in lib.rt_last_error(), (what, lib.rt_last_error())
    for mode in (abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_MODE_VECTORIZED3,
                 F32 | abi.RT_FLAG_ROOT2 | abi.RT_FLAG_MODE_SCALAR):
        assert scatter(lib, ctx, 64, p, None, p, p, p, p, p, 0, mode, p, p, p) == abi.RT_ERR_UNSUPPORTED, mode
        assert b"rt_scatter_async" in lib.rt_last_error()
    for flags in (F32, F32 | abi.RT_FLAG_ROOT2):   # the fp32 counter's bounce limit, checked at the call
        assert scatter(lib, ctx, 64, p, None, p, p, p, p, p, abi.RT_MAX_BOUNCES_F32 + 1, flags, p, p, p) == abi.RT_ERR_UNSUPPORTED
        assert b"rt_scatter_async" in lib.rt_last_error() and b"RT_MAX_BOUNCES_F32" in lib.rt_last_error()
    for flags in (0, F32, abi.RT_FLAG_ROOT2, F32 | abi.RT_FLAG_ROOT2):   # accepted flags
        assert scatter(lib, ctx, 0x80000000, p, None, p, p, p, p, p, 3, flags, None, p, None) == abi.RT_ERR_UNSUPPORTED, flags
        assert b"rt_scatter_async" in lib.rt_last_error() and b"too many rays" in lib.rt_last_error()


def test_path_step_arguments_are_refused_without_a_gpu(lib):
    p = ctypes.c_void_p(16)
    ctx = ctypes.c_void_p(16)
    outs, none = (p, p, p, p, p), (None,) * 5
    invalid = [
        ("NULL ctx", (None, 64, p, p, p, p, p, 0, 0, outs)),
        ("NULL origins", (ctx, 64, None, p, p, p, p, 0, 0, outs)),
        ("NULL directions", (ctx, 64, p, None, p, p, p, 0, F32, outs)),
        ("NULL pixel", (ctx, 64, p, p, p, None, p, 0, 0, outs)),
        ("NULL sample", (ctx, 64, p, p, None, p, None, 0, 0, none)),
        ("unknown flag bits", (ctx, 64, p, p, p, p, p, 0, 0x40, outs)),
    ]
    for what, args in invalid:
        assert step(lib, *args) == abi.RT_ERR_INVALID, what
        assert b"rt_path_step_async" in lib.rt_last_error(), (what, lib.rt_last_error())
    for mode in (abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_MODE_VECTORIZED3,
                 F32 | abi.RT_FLAG_ROOT2 | abi.RT_FLAG_MODE_VECTORIZED):
        assert step(lib, ctx, 64, p, p, p, p, p, 0, mode, outs) == abi.RT_ERR_UNSUPPORTED, mode
        assert b"rt_path_step_async" in lib.rt_last_error()
    assert step(lib, ctx, 64, p, p, p, p, p, abi.RT_MAX_BOUNCES_F32 + 1, F32, outs) == abi.RT_ERR_UNSUPPORTED
    assert b"rt_path_step_async" in lib.rt_last_error() and b"RT_MAX_BOUNCES_F32" in lib.rt_last_error()
    for flags in (0, F32, abi.RT_FLAG_ROOT2, F32 | abi.RT_FLAG_ROOT2):
        assert step(lib, ctx, 0x80000000, p, p, None, p, p, 1, flags, none) == abi.RT_ERR_UNSUPPORTED, flags
        assert b"rt_path_step_async" in lib.rt_last_error() and b"too many rays" in lib.rt_last_error()


@pytest.mark.parametrize("name", ["rt_scatter_async", "rt_path_step_async"])
def test_no_scene_is_refused_before_any_device_work(name):
    """A context that never saw a scene: RT_ERR_INVALID, named (rt_context_create needs a device, so the GPU suite
    covers the refusal itself).  Here: the order of the checks in the source puts every one ahead of begin_launch."""
    src = open(abi.SOURCE_FILES[0]).read()
    body = src[src.index(f'extern "C" int {name}('):]
    body = body[:body.index("\n}\n")]
    assert body.index("NULL argument") < body.index("check_step(") < body.index("n_rays == 0") < body.index("begin_launch")
    shared = src[src.index("static int check_step("):]
    shared = shared[:shared.index("\n}\n")]
    for text in ("unknown flag bits", "no RT_FLAG_MODE_*", "RT_MAX_BOUNCES_F32", "too many rays", "no scene set"):
        assert text in shared, text
    assert "hip" not in shared


# ---------------------------------------------------------------- the renderer's own checks
D8 = np.zeros((8, 3))
I8, T8 = np.zeros(8, np.int32), np.zeros(8)


@pytest.mark.parametrize("flags", [abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, F32 | abi.RT_FLAG_MODE_VECTORIZED3])
def test_the_methods_refuse_the_mode_renderers_before_touching_the_context(flags):
    r = NoGpu(flags)   # no ctx, no lib, no seed: any use of them raises AttributeError
    u = FakeDevice(np.zeros(8, np.uint32))
    with pytest.raises(ValueError, match="live path"):
        r.scatter(np.zeros(3), D8, I8, T8, None)
    with pytest.raises(ValueError, match="live path"):
        r.scatter_into(np.zeros(3), FakeDevice(D8), FakeDevice(I8), FakeDevice(T8), u, u)
    with pytest.raises(ValueError, match="live path"):
        r.path_step(D8, D8, None)
    with pytest.raises(ValueError, match="live path"):
        r.path_step_into(FakeDevice(D8), FakeDevice(D8), u, u)


def test_scatter_and_path_step_refuse_bad_arguments_before_any_gpu_call():
    r = NoGpu(F32)
    for o, d in ((np.zeros(3), np.zeros((8, 2))), (np.zeros(3), np.zeros(8)), (np.zeros((7, 3)), D8), (np.zeros(4), D8)):
        with pytest.raises(ValueError, match="shape"):
            r.scatter(o, d, I8, T8, None)
    with pytest.raises(ValueError, match="shape"):
        r.path_step(np.zeros(3), D8, None)   # no shared origin: the step writes the origins back
    with pytest.raises(ValueError, match="shape"):
        r.path_step(np.zeros((7, 3)), D8, None)
    for bad_i in (np.zeros(7, np.int32), np.zeros(8), np.zeros((8, 1), np.int32)):
        with pytest.raises(ValueError, match="index"):
            r.scatter(np.zeros(3), D8, bad_i, T8, None)
    with pytest.raises(ValueError, match="int32"):
        r.scatter(np.zeros(3), D8, np.full(8, 1 << 31), T8, None)
    for bad_t in (np.zeros(9), np.zeros(8, complex)):
        with pytest.raises(ValueError, match="t must be"):
            r.scatter(np.zeros(3), D8, I8, bad_t, None)
    for kw in (dict(pixel=np.zeros(7, int)), dict(sample=np.zeros(8)), dict(pixel=np.full(8, -1)), dict(sample=np.full(8, 1 << 32)),
               dict(colour=np.zeros((8, 2))), dict(colour=np.zeros((8, 3), complex)), dict(bounce=-1), dict(bounce=1.5),
               dict(bounce=abi.RT_MAX_BOUNCES_F32 + 1), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.0)):
        with pytest.raises(ValueError):
            r.scatter(np.zeros(3), D8, I8, T8, None, **kw)
        with pytest.raises(ValueError):
            r.path_step(D8, D8, None, **kw)
    with pytest.raises(ValueError, match="unknown path-step output"):
        NoGpu(F32 | 0).path_step(D8, D8, None, seed=1, want=("status", "point"))
    # what the checks hand on
    o, d, shared, i, t, pix, smp, col, b = checks.check_scatter(F32 | abi.RT_FLAG_ROOT2, [1, 2, 3], D8, I8.astype(np.int64),
                                                                T8, colour=np.ones((8, 3)), bounce=np.int64(5))
    assert shared and o.dtype == np.float64 and d.dtype == np.float32 and i.dtype == np.int32 and t.dtype == np.float32
    assert pix.tolist() == list(range(8)) and not smp.any() and pix.dtype == smp.dtype == np.uint32
    assert col.dtype == np.float32 and b == 5 and isinstance(b, int)
    assert checks.check_scatter(0, D8, D8, I8, T8)[7] is None and checks.check_scatter(0, D8, D8, I8, T8, bounce=10 ** 6)[8] == 10 ** 6
    src = np.ones((8, 3))
    o, d, pix, smp, col, b = checks.check_path_step(0, src, src, sample=np.arange(8), colour=src)
    assert all(a is not src and a.flags.c_contiguous for a in (o, d, col)) and smp.tolist() == list(range(8))
    assert rmod.check_scatter is checks.check_scatter and rmod.check_path_step is checks.check_path_step
    # the ray checks are check_query's own, reused: the same refusal, word for word
    with pytest.raises(ValueError, match=r"directions must have shape \(n, 3\), not \(8, 2\)"):
        checks.check_scatter(0, np.zeros(3), np.zeros((8, 2)), I8, T8)


def test_the_into_methods_refuse_bad_arrays_before_any_gpu_call():
    r = NoGpu(F32, device=0)
    d = FakeDevice(np.zeros((8, 3), np.float32))
    o = FakeDevice(np.zeros((8, 3), np.float32))
    i, t = FakeDevice(np.zeros(8, np.int32)), FakeDevice(np.zeros(8, np.float32))
    u = FakeDevice(np.zeros(8, np.uint32))
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        r.scatter_into(o, np.zeros((8, 3), np.float32), i, t, u, u)
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        r.scatter_into(o, d, np.zeros(8, np.int32), t, u, u)
    with pytest.raises(TypeError, match="origins"):
        r.path_step_into(np.zeros(3), d, u, u)
    for bad in (dict(index=FakeDevice(np.zeros(8, np.int64))), dict(t=FakeDevice(np.zeros(8))), dict(pixel=FakeDevice(np.zeros(8, np.int32))),
                dict(sample=FakeDevice(np.zeros(8, np.uint64)))):
        args = dict(index=i, t=t, pixel=u, sample=u)
        args.update(bad)
        with pytest.raises(ValueError, match="dtype"):
            r.scatter_into(o, d, args["index"], args["t"], args["pixel"], args["sample"])
    with pytest.raises(ValueError, match="shape"):
        r.scatter_into(o, d, i, t, u, u, colour=FakeDevice(np.zeros((8, 4), np.float32)))
    with pytest.raises(ValueError, match="shape"):
        r.scatter_into(o, d, i, t, u, u, out_origins=FakeDevice(np.zeros((7, 3), np.float32)))
    with pytest.raises(ValueError, match="read-only"):
        r.scatter_into(o, d, i, t, u, u, out_directions=FakeDevice(np.zeros((8, 3), np.float32), readonly=True))
    with pytest.raises(ValueError, match="read-only"):   # in place: the inputs are the outputs
        r.scatter_into(o, FakeDevice(np.zeros((8, 3), np.float32), readonly=True), i, t, u, u)
    with pytest.raises(ValueError, match="read-only"):
        r.path_step_into(FakeDevice(np.zeros((8, 3), np.float32), readonly=True), d, u, u)
    with pytest.raises(ValueError, match="dtype"):
        r.path_step_into(o, d, u, u, status=FakeDevice(np.zeros(8, np.int8)))
    with pytest.raises(ValueError, match="shape"):
        r.path_step_into(o, d, u, u, normal=FakeDevice(np.zeros(8, np.float32)))
    with pytest.raises(ValueError, match="contiguous"):
        r.path_step_into(o, d, u, u, front=FakeDevice(np.zeros(16, np.uint8)[::2]))
    with pytest.raises(ValueError, match="device"):
        r.path_step_into(o, d, u, FakeDevice(np.zeros(8, np.uint32), device=Dev("cuda", 1)))
    r.seed = 1
    with pytest.raises(TypeError, match="stream"):
        r.path_step_into(o, d, u, u, stream="0")
    with pytest.raises(TypeError, match="stream"):
        r.scatter_into(o, d, i, t, u, u, stream=1.5)
    # what the checks hand on: in place by default; a shared origin writes no origins unless asked
    got = checks.check_scatter_into(F32, 0, o, d, i, t, u, u, None, None, None, 3)
    assert got[0] == 8 and got[1] == got[9] == o.a.ctypes.data and got[3] == got[10] == d.a.ctypes.data and got[8] is None
    got = checks.check_scatter_into(F32, 0, [1, 2, 3], d, i, t, u, u, None, None, None)
    assert got[1] is None and got[2].dtype == np.float64 and got[9] is None and got[10] == d.a.ctypes.data
    n, d_org, d_dir, d_col, d_pix, d_smp, ptrs, b = checks.check_path_step_into(
        F32, 0, o, d, u, u, None, dict(status=FakeDevice(np.zeros(8, np.uint8)), index=None, t=t, normal=None, front=None), 2)
    assert n == 8 and d_org == o.a.ctypes.data and d_col is None and sorted(ptrs) == ["status", "t"] and b == 2


def test_every_raise_of_the_step_checks_is_reached_and_worded():
    """tests/test_renderer_messages.py's bar for the new module: each raise statement of step_checks.py is the end of a
    call below, and its type and full text are pinned."""
    r = NoGpu(F32, device=0)
    r.seed = 1
    r._scene_flat = None
    d = FakeDevice(np.zeros((8, 3), np.float32))
    i, t = FakeDevice(np.zeros(8, np.int32)), FakeDevice(np.zeros(8, np.float32))
    u = FakeDevice(np.zeros(8, np.uint32))
    S = lambda **kw: r.scatter(np.zeros(3), D8, kw.pop("index", I8), kw.pop("t", T8), None, **kw)   # noqa: E731
    cases = [
        (lambda: r.path_step(D8, D8, None, want=("point",)), ValueError,
         "unknown path-step output 'point' (one of ['status', 'index', 't', 'normal', 'front'])"),
        (lambda: S(bounce=-1), ValueError, "bounce must be an integer in 0..2^32 - 1, not -1"),
        (lambda: S(bounce=3840), ValueError, "an fp32 renderer scatters bounces 0..3839 only, not 3840"),
        (lambda: S(seed=-1), ValueError, "seed must be an integer in 0..2^64 - 1 or None, not -1"),
        (lambda: S(pixel=np.zeros(8)), ValueError, "pixel must be integers, not dtype float64"),
        (lambda: S(sample=np.zeros(7, int)), ValueError, "sample must have shape (8,), one per ray, not (7,)"),
        (lambda: S(pixel=np.full(8, -1)), ValueError, "pixel must lie in 0..2^32 - 1"),
        (lambda: S(colour=np.zeros((8, 3), complex)), ValueError, "colour must be numbers, not dtype complex128"),
        (lambda: S(colour=np.zeros((8, 2))), ValueError, "colour must have shape (8, 3), one per ray, not (8, 2)"),
        (lambda: S(index=np.zeros(7, np.int32)), ValueError, "index must be (8,) integers, a query's index, not int32 (7,)"),
        (lambda: S(index=np.full(8, 1 << 31)), ValueError, "index must fit int32"),
        (lambda: S(t=np.zeros(9)), ValueError, "t must be (8,) numbers, a query's t, not float64 (9,)"),
        (lambda: r.path_step(np.zeros(3), D8, None), ValueError,
         "origins must have the shape of directions, one per ray (the step writes them back), not (3,)"),
        (lambda: r.path_step_into(np.zeros(3), d, u, u), TypeError,
         "origins must be a device array of shape (n, 3): the step writes the origins back"),
        (lambda: r.scatter_into(np.zeros(3), d, i, t, u, u), RuntimeError, "scatter_into needs a scene: call set_scene first"),
    ]
    path = checks.__file__
    hit = set()
    for call, kind, text in cases:
        with pytest.raises(kind) as e:
            call()
        assert str(e.value) == text
        hit |= {f.lineno for f in traceback.extract_tb(e.value.__traceback__) if f.filename == path}
    source = open(path).read()
    raises = [n for n in ast.walk(ast.parse(source)) if isinstance(n, ast.Raise)]
    assert len(raises) == len(cases)
    for n in raises:
        assert any(n.lineno <= line <= n.end_lineno for line in hit), ast.get_source_segment(source, n)
