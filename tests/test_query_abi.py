"""rt_query_hits_async, GpuRenderer.query and query_into: what can be checked without a GPU.  The entry point checks
its arguments before any HIP call, so every refusal below happens on a machine without a device; the renderer checks
shapes, dtypes, names and modes before it touches its context; and the launches tests/test_gpu_query.py sends
(tests/query_cases.py) are checked here with the oracle alone, so that the GPU test cannot pass vacuously.

The launch conditions, per launch and per mode (packed: quirk Q1; root2):
  * at least a quarter of the valid rays hit;
  * at least one valid ray misses.  One exception, by construction of tests/cull_cases.py: camera:inside under root2.
    Its centre lies inside the closed shell sphere, so with the far root accepted every ray hits the shell or
    something nearer; there the share of hits is asserted to be at least 0.95 instead;
  * no target sphere is left without a hit: every sphere a valid ray was aimed at is the reference's nearest hit of
    at least one ray aimed at it.  cull_cases aims about eight grazing rays at a target, two thirds of them outside
    it, so a target's grazing rays may all rightly miss; query_cases.with_coverage therefore appends one ray per
    case straight at the target's centre (and one wave of misses).  One exception, again by construction: the small
    spheres inside the shell (scene indices 2 .. 9), for rays that start outside the shell (the graze family):
    the shell is the nearer hit.  They are reached by the camera:inside family, whose targets they are.
"""
import ctypes
import re

import numpy as np
import pytest

import cull_cases as cc
import query_cases as qc
import rt_mi355x as rt
from rt_mi355x import abi
from rt_mi355x import renderer as rmod
from test_abi import declared_functions

HEADER = abi.SOURCE_FILES[-1]


# ---------------------------------------------------------------- the header and the binding
def test_symbol_is_exported_and_declared():
    assert "rt_query_hits_async" in abi.EXPORTED and "rt_memcpy_h2d" in abi.EXPORTED
    assert sorted(abi.EXPORTED) == declared_functions()   # test_abi.py's equality, with the new symbols
    text = open(HEADER).read()
    assert "int rt_query_hits_async(rt_context* ctx, uint64_t n_rays, const void* d_origins, const double* origin," in text
    assert "rt_query.hpp" in abi.KERNEL_SOURCES and abi.KERNEL_SOURCES[-1] == "rt_query.hpp"
    assert abi.source_hash() and "query_rays" in abi.kernel_source_text()


def test_header_states_the_definition():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    i = text.index("ray queries: the closest hit of caller-supplied rays")
    doc = text[i:text.index("int rt_query_hits_async(", i)]
    for phrase in ("t in [0.001, inf)", "ties go to the later sphere", "quirk Q1 applies", "unless RT_FLAG_ROOT2",
                   "Picking wants RT_FLAG_ROOT2", "Directions are NOT normalised", "index -1, t +inf",
                   "index -2 (RT_QUERY_INVALID), t NaN", "outside [1e-6, 1e6]", "The bounds themselves are valid",
                   "no FMA", "front    pk_dot(d, normal) < 0", "negated when not front",
                   "A value does not depend on which other outputs were asked for", "n_rays > 0x7FFFFFFF",
                   "samples = ray_segments = the valid rays", "bounce_iters = 0"):
        assert phrase in doc, phrase
    assert re.search(r"#define RT_QUERY_INVALID \(-2\)", text) and re.search(r"#define RT_QUERY_MISS \(-1\)", text)
    assert abi.RT_QUERY_INVALID == -2 and abi.RT_QUERY_MISS == -1


def call(lib, ctx, n, d_origins, origin, d_dirs, flags, outs):
    o3 = None if origin is None else (ctypes.c_double * 3)(*origin)
    return lib.rt_query_hits_async(ctx, n, d_origins, o3, d_dirs, flags, *outs, None)


def test_arguments_are_refused_without_a_gpu(lib):
    p = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    outs, none = (p, p, p, p, p), (None,) * 5
    O = (1.0, 2.0, 3.0)
    invalid = [
        ("NULL ctx", (None, 64, p, None, p, 0, outs)),
        ("NULL directions", (ctx, 64, p, None, None, 0, outs)),
        ("all outputs NULL", (ctx, 64, p, None, p, 0, none)),
        ("both origin forms", (ctx, 64, p, O, p, 0, outs)),
        ("neither origin form", (ctx, 64, None, None, p, 0, outs)),
        ("unknown flag bits", (ctx, 64, p, None, p, 0x20, outs)),
        ("unknown flag bits with F32", (ctx, 64, None, O, p, abi.RT_FLAG_F32 | 0x100, outs)),
    ]
    for what, args in invalid:
        assert call(lib, *args) == abi.RT_ERR_INVALID, what
        assert b"rt_query_hits_async" in lib.rt_last_error(), (what, lib.rt_last_error())
    for mode in (abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_MODE_VECTORIZED3,
                 abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2 | abi.RT_FLAG_MODE_SCALAR):
        assert call(lib, ctx, 64, p, None, p, mode, outs) == abi.RT_ERR_UNSUPPORTED, mode
        assert b"rt_query_hits_async" in lib.rt_last_error()
    for flags in (0, abi.RT_FLAG_F32, abi.RT_FLAG_ROOT2, abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2):   # accepted flags
        assert call(lib, ctx, 0x80000000, p, None, p, flags, outs) == abi.RT_ERR_UNSUPPORTED, flags
        assert b"too many rays" in lib.rt_last_error()
    assert lib.rt_memcpy_h2d(None, p, p, 4) == abi.RT_ERR_INVALID and b"rt_memcpy_h2d" in lib.rt_last_error()


def test_kernel_query_bit_decodes_alike_in_c_and_python():
    text = open(HEADER).read()
    m = re.search(r"#define RT_KERNEL_QUERY\(id\) \(\(\(id\) >> (\d+)\) & 1u\)", text)
    assert m and int(m.group(1)) == 12
    q = 0x8000 | 1 << 12
    for kid in (q, q | 1 | 4 << 1 | 1 << 7, q | 5 << 1 | 1 << 8 | 1 << 4, 0x808C, 0x81F9, 0x8000 | 1 << 9 | 1 << 10,
                0x8000 | 1 << 11 | 1 | 4 << 1):
        k = abi.kernel_info(kid)
        assert abi.RT_KERNEL_QUERY(kid) == (kid >> 12) & 1 and k["query"] == bool(abi.RT_KERNEL_QUERY(kid))
    assert abi.kernel_name(q | 1 | 4 << 1 | 1 << 7) == "query_rays<double,false,true,false>"
    assert abi.kernel_name(q | 5 << 1 | 1 << 8 | 1 << 4) == "query_rays<float,true,false,true>"
    # existing names are unchanged
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"
    assert abi.kernel_name(0x81F9) == "trace_paths<double,4,true,3,true,true>"
    assert abi.kernel_name(0x8000 | 1 << 11 | 1 | 4 << 1 | 1 << 7) == "guide_pixels<double,true,false>"
    assert abi.kernel_name(0x8000 | 1 << 9 | 1 << 10 | 5 << 1) == "trace_paths_items<float,5,false,false>"
    assert abi.kernel_name(0x8000 | 1 << 9 | 1 | 4 << 1 | 1 << 8) == "trace_paths_split<double,4,false,true>"
    assert abi.kernel_info(0) is None


# ---------------------------------------------------------------- the renderer's own checks
class NoGpu(rmod.GpuRenderer):   # any use of the context or the library would raise AttributeError
    def __init__(self, flags, device=0):
        self.flags, self.device = flags, device

    def __del__(self):
        pass


D8 = np.zeros((8, 3))


@pytest.mark.parametrize("flags", [abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR,
                                   abi.RT_FLAG_F32 | abi.RT_FLAG_MODE_VECTORIZED3])
def test_query_refuses_modes_before_any_gpu_call(flags):
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).query(np.zeros(3), D8, None)
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).query_into(np.zeros(3), FakeDevice(D8))


def test_query_refuses_bad_shapes_names_and_dtypes_before_any_gpu_call():
    r = NoGpu(abi.RT_FLAG_F32)
    for o, d in ((np.zeros(3), np.zeros((8, 2))), (np.zeros(3), np.zeros(8)), (np.zeros(3), np.zeros((2, 8, 3))),
                 (np.zeros((7, 3)), D8), (np.zeros(4), D8), (np.zeros((8, 3, 1)), D8), (np.zeros((3, 8)), D8)):
        with pytest.raises(ValueError, match="shape"):
            r.query(o, d, None)
    with pytest.raises(ValueError, match="numbers"):
        r.query(np.zeros(3), np.zeros((8, 3), dtype=complex), None)
    with pytest.raises(ValueError, match="numbers"):
        r.query(np.array(["a", "b", "c"]), D8, None)
    with pytest.raises(ValueError, match="unknown query output"):
        r.query(np.zeros(3), D8, None, want=("t", "normals"))
    with pytest.raises(ValueError, match="no query output"):
        r.query(np.zeros(3), D8, None, want=())
    assert rmod.QUERY_NAMES == ("t", "index", "normal", "point", "front")
    # what the checks hand on: the renderer's precision, a shared origin kept in double
    o, d, shared, want = rmod.check_query(abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2, [1, 2, 3], np.zeros((8, 3), np.float64))
    assert shared and o.dtype == np.float64 and d.dtype == np.float32 and d.flags.c_contiguous and want == rmod.QUERY_NAMES
    o, d, shared, _ = rmod.check_query(0, np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32)[::-1])
    assert not shared and o.dtype == d.dtype == np.float64 and d.flags.c_contiguous


class FakeDevice:
    """An object with __cuda_array_interface__ over a numpy array's memory (never dereferenced by the checks)."""

    def __init__(self, a, readonly=False, device=None):
        self.a = a
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": a.dtype.str, "data": (a.ctypes.data or 1, readonly),
                                         "version": 3, "strides": None if a.flags.c_contiguous else a.strides}
        if device is not None:
            self.device = device


class Dev:
    def __init__(self, type_, index):
        self.type, self.index = type_, index

    def __str__(self):
        return f"{self.type}:{self.index}"


def test_query_into_refuses_bad_arrays_before_any_gpu_call():
    r = NoGpu(abi.RT_FLAG_F32, device=0)
    d = np.zeros((8, 3), np.float32)
    good = dict(t=FakeDevice(np.zeros(8, np.float32)))
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        r.query_into(np.zeros(3), d, **good)                      # a host array
    with pytest.raises(ValueError, match="dtype"):
        r.query_into(np.zeros(3), FakeDevice(np.zeros((8, 3))), **good)   # float64 in an fp32 renderer
    with pytest.raises(ValueError, match="shape"):
        r.query_into(np.zeros(3), FakeDevice(np.zeros((8, 4), np.float32)), **good)
    with pytest.raises(ValueError, match="shape"):
        r.query_into(FakeDevice(np.zeros((7, 3), np.float32)), FakeDevice(d), **good)
    with pytest.raises(ValueError, match="origins"):
        r.query_into(np.zeros(2), FakeDevice(d), **good)
    with pytest.raises(ValueError, match="contiguous"):
        r.query_into(np.zeros(3), FakeDevice(np.zeros((8, 6), np.float32)[:, ::2]), **good)
    with pytest.raises(ValueError, match="contiguous"):
        r.query_into(np.zeros(3), FakeDevice(d), t=FakeDevice(np.zeros(16, np.float32)[::2]))
    with pytest.raises(ValueError, match="dtype"):
        r.query_into(np.zeros(3), FakeDevice(d), index=FakeDevice(np.zeros(8, np.int64)))
    with pytest.raises(ValueError, match="dtype"):
        r.query_into(np.zeros(3), FakeDevice(d), front=FakeDevice(np.zeros(8, np.bool_)))
    with pytest.raises(ValueError, match="shape"):
        r.query_into(np.zeros(3), FakeDevice(d), normal=FakeDevice(np.zeros(8, np.float32)))
    with pytest.raises(ValueError, match="shape"):
        r.query_into(np.zeros(3), FakeDevice(d), t=FakeDevice(np.zeros((8, 1), np.float32)))
    with pytest.raises(ValueError, match="read-only"):
        r.query_into(np.zeros(3), FakeDevice(d), t=FakeDevice(np.zeros(8, np.float32), readonly=True))
    with pytest.raises(ValueError, match="device"):
        r.query_into(np.zeros(3), FakeDevice(d, device=Dev("cuda", 1)), **good)
    with pytest.raises(ValueError, match="device"):
        r.query_into(np.zeros(3), FakeDevice(d), t=FakeDevice(np.zeros(8, np.float32), device=Dev("cpu", None)))
    with pytest.raises(ValueError, match="no query output"):
        r.query_into(np.zeros(3), FakeDevice(d))
    with pytest.raises(TypeError, match="stream"):
        r.query_into(np.zeros(3), FakeDevice(d, device=Dev("cuda", 0)), stream="0", **good)
    n, d_org, origin, d_dir, ptrs = rmod.check_query_into(abi.RT_FLAG_F32, 0, [1, 2, 3], FakeDevice(d), dict(
        t=FakeDevice(np.zeros(8, np.float32)), index=FakeDevice(np.zeros(8, np.int32)), normal=None,
        point=FakeDevice(np.zeros((8, 3), np.float32)), front=FakeDevice(np.zeros(8, np.uint8))))
    assert n == 8 and d_org is None and origin.dtype == np.float64 and d_dir == d.ctypes.data
    assert sorted(ptrs) == ["front", "index", "point", "t"]


# ---------------------------------------------------------------- the precondition, restated
def test_valid_rays_is_the_headers_precondition():
    for dtype in (np.float32, np.float64):
        t = dtype
        lo, hi = t(1e-6), t(1e6)
        d = np.array([[1, 0, 0], [0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 1], [0, -np.inf, 1], [1e3, 0, 0], [1e-3, 0, 0],
                      [np.sqrt(lo), 0, 0], [0, np.sqrt(hi), 0], [1001, 0, 0], [9.99e-4, 0, 0], [600, 600, 600]], dtype)
        ok = qc.valid_rays(np.zeros(3), d)
        a = (d.astype(np.float64) ** 2).sum(1)
        want = np.isfinite(d).all(1) & (a.astype(dtype) >= lo) & (a.astype(dtype) <= hi)   # one term each: exact products
        want[11] = False   # three terms: 1.08e6
        assert ok.tolist() == want.tolist(), dtype
        assert ok[0] and not ok[1:5].any() and not ok[9:].any()
        assert np.array_equal(qc.valid_fast(np.zeros(3), d), ok)
        o = np.zeros((12, 3), dtype)
        o[0, 1] = np.inf
        assert not qc.valid_rays(o, d)[0] and not qc.valid_fast(o, d)[0]


# ---------------------------------------------------------------- the GPU test's launches, with the oracle alone
INNER = set(range(cc.SHELL + 1, cc.SHELL + 1 + cc.N_INNER))


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("fam", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.SCENES)
def test_launches(name, fam, kind, prec):
    la = qc.launch(name, fam, prec, kind)
    dtype = cc.DTYPES[prec]
    assert la.o.dtype == la.d.dtype == dtype and la.o.shape == la.d.shape == (la.n, 3) and la.n % 64 == 0
    base = cc.compose(la.sc, fam, dtype, kind)   # cull_cases' rays, unchanged, lead the launch
    nb = base.rays.n
    act = base.active.astype(bool)
    assert np.array_equal(la.d[:nb][act], base.rays.d.T[act]) and np.array_equal(la.o[:nb], base.rays.o.T)
    assert np.isnan(la.d[:nb][~act]).all() and not la.valid[:nb][~act].any()
    if kind == "solo":   # one valid lane per wave, NaN directions around it
        assert (la.valid[:nb].reshape(-1, 64).sum(1) == 1).all()
    else:                # all but the few rays longer than 1e3 (cull_cases.misses scales |d| up to 1.2e3)
        assert la.valid[:nb].mean() > 0.99
    assert np.array_equal(la.valid, qc.valid_rays(la.o, la.d))   # the exact restatement, ray by ray
    assert (la.centre is not None) == fam.startswith("camera")
    if la.centre is not None:
        assert (la.o == la.centre[None, :]).all()
    v = la.valid
    for mode in qc.MODES:
        idx, t = la.ref[mode]
        assert (idx[~v] == qc.INVALID).all() and np.isnan(t[~v]).all()
        assert (idx[v] >= qc.MISS).all() and np.isinf(t[v][idx[v] == qc.MISS]).all() and np.isfinite(t[v][idx[v] >= 0]).all()
        hits, misses = (idx[v] >= 0).mean(), int((idx[v] == qc.MISS).sum())
        targets = set(la.target[la.target >= 0].tolist())
        reached = set(idx[(la.target >= 0) & (idx == la.target)].tolist())
        print(name, fam, kind, prec, mode, f"valid {int(v.sum())} of {la.n}, hits {hits:.3f}, misses {misses}, "
              f"targets {len(targets)}, not reached {sorted(targets - reached)}")
        assert hits >= 0.25, mode
        if fam == "camera:inside" and mode == "root2":
            assert hits >= 0.95, mode
        else:
            assert misses >= 1, mode
        unreachable = INNER if fam == "graze" else set()
        assert targets - reached <= unreachable, (mode, sorted(targets - reached))
        if fam in ("graze", "camera:outside_0", "camera:inside"):
            assert len(targets) >= 8
