"""rt_query_occluded_async, GpuRenderer.occluded and occluded_into: what can be checked without a GPU.  The entry
point checks its arguments before any HIP call, so every refusal below happens on a machine without a device, and the
renderer checks shapes, dtypes, t_max and modes before it touches its context (tests/test_query_abi.py's manner)."""
import ctypes
import re

import numpy as np
import pytest

from rt_mi355x import abi
from rt_mi355x import occlusion_checks as checks
from rt_mi355x import renderer as rmod
from test_abi import declared_functions
from test_query_abi import Dev, FakeDevice, NoGpu

HEADER = abi.SOURCE_FILES[-1]
NAME = b"rt_query_occluded_async"


# ---------------------------------------------------------------- the header and the binding
def test_symbol_is_exported_and_declared(lib):
    assert "rt_query_occluded_async" in abi.EXPORTED
    assert sorted(abi.EXPORTED) == declared_functions()
    assert hasattr(lib, "rt_query_occluded_async")
    text = open(HEADER).read()
    assert ("int rt_query_occluded_async(rt_context* ctx, uint64_t n_rays, const void* d_origins, const double* origin,\n"
            "                            const void* d_directions, const void* d_t_max, double t_max, uint32_t flags,\n"
            "                            void* d_occluded, void* stream);") in text
    assert abi.KERNEL_SOURCES[-1] == "rt_query.hpp" and "occlusion_rays" in abi.kernel_source_text()
    assert len(lib.rt_query_occluded_async.argtypes) == 10


def test_header_states_the_definition():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    i = text.index("occlusion queries: is anything in the way before t_max")
    assert i > text.index("int rt_query_hits_async(")   # the doc block follows that declaration
    doc = text[i:text.index("int rt_query_occluded_async(", i)]
    for phrase in ("accepted root r satisfies r < t_max, strictly", "near root when it lies in [0.001, inf)",
                   "quirk Q1 applies unless RT_FLAG_ROOT2", "closest hit of (o, d) exists and its t < t_max",
                   "Directions are NOT normalised", "d = light - p with t_max = 1", "its t_max is not NaN",
                   "t_max may be +inf (unbounded), negative, zero or -inf",
                   "t_max <= T(0.001) is never occluded and is not traced", "0 (RT_OCCLUDED_NO)", "1 (RT_OCCLUDED_YES)",
                   "255 (RT_OCCLUDED_INVALID)", "No ray's value depends on any other ray", "Both forms run the general sweep",
                   "give identical bytes", "when given the host t_max is not read", "n_rays > 0x7FFFFFFF",
                   "d_t_max NULL and the host t_max NaN", "samples = ray_segments = the valid rays", "bounce_iters = 0",
                   "RT_KERNEL_OCCLUSION(kernel_id) is set"):
        assert phrase in doc, phrase
    for name, value in (("RT_OCCLUDED_NO", 0), ("RT_OCCLUDED_YES", 1), ("RT_OCCLUDED_INVALID", 255)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(abi, name) == value
    # the query's own block now points here for what it leaves out
    q = text[text.index("ray queries: the closest hit of caller-supplied rays"):text.index("int rt_query_hits_async(")]
    assert "rt_query_occluded_async" in q and "Out of scope" in q


def test_kernel_occlusion_bit_decodes_alike_in_c_and_python():
    text = open(HEADER).read()
    m = re.search(r"#define RT_KERNEL_OCCLUSION\(id\) \(\(\(id\) >> (\d+)\) & 1u\)", text)
    assert m and int(m.group(1)) == 14
    o = 0x8000 | 1 << 14
    for kid in (o, o | 1 | 4 << 1, o | 5 << 1 | 1 << 8 | 1 << 4, 0x808C, 0x8000 | 1 << 12 | 1 << 7, 0x8000 | 1 << 13):
        assert abi.RT_KERNEL_OCCLUSION(kid) == (kid >> 14) & 1
        assert abi.kernel_info(kid)["occlusion"] == bool((kid >> 14) & 1)
    assert abi.kernel_name(o | 1 | 4 << 1) == "occlusion_rays<double,false,false>"
    assert abi.kernel_name(o | 5 << 1 | 1 << 8 | 1 << 4) == "occlusion_rays<float,true,true>"
    assert abi.kernel_name(o | 5 << 1 | 1 << 8) == "occlusion_rays<float,false,true>"
    # existing names are unchanged
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"
    assert abi.kernel_name(0x8000 | 1 << 12 | 1 | 4 << 1 | 1 << 7) == "query_rays<double,false,true,false>"
    assert abi.kernel_name(0x8000 | 1 << 13 | 6 << 1) == "trace_paths_rays<float,6,false,false>"


# ---------------------------------------------------------------- the entry point's refusals
def call(lib, ctx, n, d_origins, origin, d_dirs, d_t_max, t_max, flags, d_occ):
    o3 = None if origin is None else (ctypes.c_double * 3)(*origin)
    return lib.rt_query_occluded_async(ctx, n, d_origins, o3, d_dirs, d_t_max, t_max, flags, d_occ, None)


def test_arguments_are_refused_without_a_gpu(lib):
    p = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    O = (1.0, 2.0, 3.0)
    nan, inf = float("nan"), float("inf")
    invalid = [
        ("NULL ctx", (None, 64, p, None, p, None, inf, 0, p)),
        ("NULL directions", (ctx, 64, p, None, None, None, inf, 0, p)),
        ("NULL occluded", (ctx, 64, p, None, p, None, inf, 0, None)),
        ("both origin forms", (ctx, 64, p, O, p, None, inf, 0, p)),
        ("neither origin form", (ctx, 64, None, None, p, None, inf, 0, p)),
        ("NaN t_max without d_t_max", (ctx, 64, p, None, p, None, nan, 0, p)),
        ("NaN t_max without d_t_max, shared, f32", (ctx, 64, None, O, p, None, nan, abi.RT_FLAG_F32, p)),
        ("unknown flag bits", (ctx, 64, p, None, p, None, inf, 0x20, p)),
        ("unknown flag bits with F32", (ctx, 64, None, O, p, p, 1.0, abi.RT_FLAG_F32 | 0x100, p)),
    ]
    for what, args in invalid:
        assert call(lib, *args) == abi.RT_ERR_INVALID, what
        assert NAME in lib.rt_last_error(), (what, lib.rt_last_error())
    for mode in (abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_MODE_VECTORIZED3,
                 abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2 | abi.RT_FLAG_MODE_SCALAR):
        assert call(lib, ctx, 64, p, None, p, None, inf, mode, p) == abi.RT_ERR_UNSUPPORTED, mode
        assert NAME in lib.rt_last_error()
    for flags in (0, abi.RT_FLAG_F32, abi.RT_FLAG_ROOT2, abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2):   # accepted flags
        for d_t, t in ((None, 1.0), (p, nan)):   # with d_t_max given the host t_max is not read: NaN is no refusal
            assert call(lib, ctx, 0x80000000, p, None, p, d_t, t, flags, p) == abi.RT_ERR_UNSUPPORTED, flags
            assert NAME in lib.rt_last_error() and b"too many rays" in lib.rt_last_error()


def test_no_scene_is_refused_before_any_device_work(lib):
    """A context that never saw a scene: RT_ERR_INVALID, named.  (rt_context_create needs a device, so this is the
    one refusal that the GPU suite covers: tests/test_gpu_occlusion.py::test_refusals_on_a_live_context.)  Here: the
    order of the checks in the source puts it ahead of begin_launch."""
    src = open(abi.SOURCE_FILES[0]).read()
    body = src[src.index('extern "C" int rt_query_occluded_async('):]
    body = body[:body.index("\n}\n")]
    assert body.index("no scene set") < body.index("n_rays == 0") < body.index("begin_launch")
    for text in ("NULL argument", "exactly one of d_origins", "t_max is NaN", "unknown flag bits", "too many rays"):
        assert body.index(text) < body.index("begin_launch"), text


# ---------------------------------------------------------------- the renderer's own checks
D8 = np.zeros((8, 3))


@pytest.mark.parametrize("flags", [abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR,
                                   abi.RT_FLAG_F32 | abi.RT_FLAG_MODE_VECTORIZED3])
def test_occluded_refuses_modes_before_any_gpu_call(flags):
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).occluded(np.zeros(3), D8, None)
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).occluded_into(np.zeros(3), FakeDevice(D8), FakeDevice(np.zeros(8, np.uint8)))


def test_occluded_refuses_bad_arguments_before_any_gpu_call():
    r = NoGpu(abi.RT_FLAG_F32)
    for o, d in ((np.zeros(3), np.zeros((8, 2))), (np.zeros(3), np.zeros(8)), (np.zeros(3), np.zeros((2, 8, 3))),
                 (np.zeros((7, 3)), D8), (np.zeros(4), D8), (np.zeros((8, 3, 1)), D8), (np.zeros((3, 8)), D8)):
        with pytest.raises(ValueError, match="shape"):
            r.occluded(o, d, None)
    with pytest.raises(ValueError, match="numbers"):
        r.occluded(np.zeros(3), np.zeros((8, 3), dtype=complex), None)
    with pytest.raises(ValueError, match="numbers"):
        r.occluded(np.array(["a", "b", "c"]), D8, None)
    for bad in (np.zeros(7), np.zeros(9), np.zeros((8, 1)), np.zeros((1, 8)), np.zeros(0)):   # a bad t_max length
        with pytest.raises(ValueError, match="t_max must be a number or have shape"):
            r.occluded(np.zeros(3), D8, None, t_max=bad)
    with pytest.raises(ValueError, match="t_max is NaN"):
        r.occluded(np.zeros(3), D8, None, t_max=float("nan"))
    with pytest.raises(ValueError, match="t_max is NaN"):
        r.occluded(np.zeros(3), D8, None, t_max=np.float32("nan"))
    for bad in ("1.0", 1j, np.array(["a"] * 8), np.zeros(8, complex)):
        with pytest.raises(ValueError, match="t_max must be a number"):
            r.occluded(np.zeros(3), D8, None, t_max=bad)
    # what the checks hand on: the renderer's precision, a shared origin kept in double, t_max a float or an array
    o, d, shared, t = checks.check_occluded(abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2, [1, 2, 3], np.zeros((8, 3), np.float64), 2)
    assert shared and o.dtype == np.float64 and d.dtype == np.float32 and isinstance(t, float) and t == 2.0
    tm = np.array([1, np.nan, np.inf, -np.inf, 0, 1e300, -1, 2], np.float64)
    o, d, shared, t = checks.check_occluded(abi.RT_FLAG_F32, np.zeros((8, 3)), np.zeros((8, 3)), tm[::-1])
    assert not shared and t.dtype == np.float32 and t.flags.c_contiguous and np.isnan(t[6]) and np.isinf(t[2]) and t[2] > 0
    with np.errstate(over="ignore"):
        tm32 = tm.astype(np.float32)
    o, d, shared, t = checks.check_occluded(0, np.zeros((8, 3)), np.zeros((8, 3)), tm32)
    assert t.dtype == np.float64 and t.shape == (8,)
    assert checks.check_occluded(0, np.zeros(3), D8)[3] == np.inf
    assert checks.check_occluded(0, np.zeros(3), D8, -np.inf)[3] == -np.inf
    assert rmod.check_occluded is checks.check_occluded
    # the ray checks are check_query's own, reused: the same refusal, word for word
    for call in (checks.check_occluded, rmod.check_query):
        with pytest.raises(ValueError, match=r"directions must have shape \(n, 3\), not \(8, 2\)"):
            call(0, np.zeros(3), np.zeros((8, 2)))


def test_occluded_into_refuses_bad_arrays_before_any_gpu_call():
    r = NoGpu(abi.RT_FLAG_F32, device=0)
    d = np.zeros((8, 3), np.float32)
    occ = FakeDevice(np.zeros(8, np.uint8))
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        r.occluded_into(np.zeros(3), d, occ)                                   # host directions
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        r.occluded_into(np.zeros(3), FakeDevice(d), np.zeros(8, np.uint8))     # a host output
    with pytest.raises(TypeError, match="t_max"):
        r.occluded_into(np.zeros(3), FakeDevice(d), occ, t_max=np.zeros(8, np.float32))   # a host t_max array
    with pytest.raises(ValueError, match="dtype"):
        r.occluded_into(np.zeros(3), FakeDevice(np.zeros((8, 3))), occ)        # float64 in an fp32 renderer
    with pytest.raises(ValueError, match="dtype"):
        r.occluded_into(np.zeros(3), FakeDevice(d), FakeDevice(np.zeros(8, np.bool_)))
    with pytest.raises(ValueError, match="dtype"):
        r.occluded_into(np.zeros(3), FakeDevice(d), occ, t_max=FakeDevice(np.zeros(8, np.float64)))
    with pytest.raises(ValueError, match="shape"):
        r.occluded_into(np.zeros(3), FakeDevice(d), FakeDevice(np.zeros(7, np.uint8)))
    with pytest.raises(ValueError, match="shape"):
        r.occluded_into(np.zeros(3), FakeDevice(d), FakeDevice(np.zeros((8, 1), np.uint8)))
    with pytest.raises(ValueError, match="shape"):
        r.occluded_into(np.zeros(3), FakeDevice(d), occ, t_max=FakeDevice(np.zeros(9, np.float32)))
    with pytest.raises(ValueError, match="shape"):
        r.occluded_into(FakeDevice(np.zeros((7, 3), np.float32)), FakeDevice(d), occ)
    with pytest.raises(ValueError, match="origins"):
        r.occluded_into(np.zeros(2), FakeDevice(d), occ)
    with pytest.raises(ValueError, match="contiguous"):
        r.occluded_into(np.zeros(3), FakeDevice(d), FakeDevice(np.zeros(16, np.uint8)[::2]))
    with pytest.raises(ValueError, match="contiguous"):
        r.occluded_into(np.zeros(3), FakeDevice(d), occ, t_max=FakeDevice(np.zeros(16, np.float32)[::2]))
    with pytest.raises(ValueError, match="read-only"):
        r.occluded_into(np.zeros(3), FakeDevice(d), FakeDevice(np.zeros(8, np.uint8), readonly=True))
    with pytest.raises(ValueError, match="device"):
        r.occluded_into(np.zeros(3), FakeDevice(d), occ, t_max=FakeDevice(np.zeros(8, np.float32), device=Dev("cuda", 1)))
    with pytest.raises(ValueError, match="t_max is NaN"):
        r.occluded_into(np.zeros(3), FakeDevice(d), occ, t_max=float("nan"))
    with pytest.raises(TypeError, match="stream"):
        r.occluded_into(np.zeros(3), FakeDevice(d, device=Dev("cuda", 0)), occ, stream="0")
    tmax = np.zeros(8, np.float32)
    n, d_org, origin, d_dir, d_t, t, d_occ = checks.check_occluded_into(abi.RT_FLAG_F32, 0, [1, 2, 3], FakeDevice(d), occ,
                                                                        FakeDevice(tmax))
    assert n == 8 and d_org is None and origin.dtype == np.float64 and d_dir == d.ctypes.data
    assert d_t == tmax.ctypes.data and d_occ == occ.a.ctypes.data
    n, d_org, origin, d_dir, d_t, t, d_occ = checks.check_occluded_into(abi.RT_FLAG_F32, 0, FakeDevice(d), FakeDevice(d), occ, 2)
    assert d_org == d.ctypes.data and origin is None and d_t is None and t == 2.0 and isinstance(t, float)


def test_every_raise_of_the_occlusion_checks_is_reached_and_worded():
    """tests/test_renderer_messages.py's bar for the new module: each raise statement of occlusion_checks.py is the
    end of a call below, and its type and full text are pinned."""
    import ast
    import traceback
    r = NoGpu(abi.RT_FLAG_F32, device=0)
    r._scene_flat = None
    d = FakeDevice(np.zeros((8, 3), np.float32))
    occ = FakeDevice(np.zeros(8, np.uint8))
    cases = [
        (lambda: r.occluded(np.zeros(3), D8, None, t_max="1.0"), ValueError,
         "t_max must be a number or an array of numbers, not dtype <U3"),
        (lambda: r.occluded(np.zeros(3), D8, None, t_max=float("nan")), ValueError,
         "t_max is NaN (a per-ray array may hold NaN: such a ray is invalid)"),
        (lambda: r.occluded(np.zeros(3), D8, None, t_max=np.zeros(7)), ValueError,
         "t_max must be a number or have shape (8,), one bound per ray, not (7,)"),
        (lambda: r.occluded_into(np.zeros(3), d, occ, t_max=np.zeros(8, np.float32)), TypeError,
         "t_max must be a number or a device array exposing __cuda_array_interface__"),
        (lambda: r.occluded_into(np.zeros(3), d, occ), RuntimeError, "occluded_into needs a scene: call set_scene first"),
    ]
    path = checks.__file__
    hit = set()
    for call, kind, text in cases:
        with pytest.raises(kind) as e:
            call()
        assert str(e.value) == text
        hit |= {f.lineno for f in traceback.extract_tb(e.value.__traceback__) if f.filename == path}
    raises = [n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Raise)]
    assert len(raises) == len(cases)
    for n in raises:
        assert any(n.lineno <= line <= n.end_lineno for line in hit), ast.get_source_segment(open(path).read(), n)
