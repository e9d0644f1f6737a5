"""rt_path_step_list_async, rt_ray_list_compact_async and GpuRenderer.path_step_list_into / compact_list_into: what can
be checked without a GPU (tests/test_step_abi.py's manner).  The entry points check their arguments before any HIP
call, so every refusal below happens on a machine without a device, and the renderer checks its arrays before it
touches its context."""
import ast
import ctypes
import re
import traceback

import numpy as np
import pytest

from rt_mi355x import abi
from rt_mi355x import list_checks as checks
from test_abi import declared_functions
from test_query_abi import Dev, FakeDevice, NoGpu

HEADER = abi.SOURCE_FILES[-1]
F32 = abi.RT_FLAG_F32
STEP = "rt_path_step_list_async"
COMPACT = "rt_ray_list_compact_async"


# ---------------------------------------------------------------- the header and the binding
def test_symbols_are_exported_and_declared(lib):
    assert STEP in abi.EXPORTED and COMPACT in abi.EXPORTED
    assert sorted(abi.EXPORTED) == declared_functions()
    assert hasattr(lib, STEP) and hasattr(lib, COMPACT)
    text = open(HEADER).read()
    assert ("int rt_path_step_list_async(rt_context* ctx, uint64_t n_rays, const void* d_list_in, const void* d_count_in,\n"
            "                            void* d_origins, void* d_directions, void* d_colour, const void* d_pixel, const void* d_sample,\n"
            "                            uint32_t bounce, uint64_t seed, uint32_t flags,\n"
            "                            void* d_status, void* d_index, void* d_t, void* d_normal, void* d_front,\n"
            "                            void* d_list_out, void* d_count_out, void* stream);") in text
    assert ("int rt_ray_list_compact_async(rt_context* ctx, uint64_t n_rays, const void* d_list_in, const void* d_count_in,\n"
            "                              const void* d_keep /* uint8 [n_rays], by ray id */,\n"
            "                              void* d_list_out, void* d_count_out, void* stream);") in text
    assert abi.KERNEL_SOURCES.index("rt_list.hpp") == abi.KERNEL_SOURCES.index("rt_step.hpp") + 1
    src = abi.kernel_source_text()
    for kernel in ("path_step_list", "keep_ballots", "list_tile_sums", "list_scan_tiles", "list_scatter"):
        assert f"void {kernel}(" in src, kernel
    assert len(lib.rt_path_step_list_async.argtypes) == 20 and len(lib.rt_ray_list_compact_async.argtypes) == 8
    makefile = open(abi.PKG_DIR + "/Makefile").read()
    assert "csrc/rt_list.hpp" in makefile   # tests/test_abi.py holds the hash's file order to the Makefile's
    # the constants Python mirrors for the tests' sizes
    assert f"kListTileDefault = {abi.LIST_TILE_DEFAULT}u" in src and f"kListScanChunk = {abi.LIST_SCAN_CHUNK}u" in src


def test_header_states_the_definitions():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    i = text.index("ray lists: path steps over the live rays only")
    assert i > text.index("int rt_path_step_async(")
    doc = text[i:text.index("int rt_path_step_list_async(", i)]
    for phrase in ("entries past count are never read", "indexed by ray id; only the list shrinks",
                   "exactly what rt_path_step_async does to ray r, bit for bit",
                   "No byte of any array is written at a ray that is not listed",   # unlisted rays untouched
                   "d_list_in NULL: the identity list", "d_count_in NULL: count = n_rays",
                   "in increasing i (stable order", "reproducible byte for byte",   # stable order
                   "kept iff d_keep[list_in[i]] != 0",
                   "a list entry >= n_rays is skipped", "a count > n_rays is clamped to n_rays",   # the bounds rule
                   "rt_context_collect returns RT_ERR_INVALID", "never fault on a bad list",
                   "A ray id listed twice is undefined for that ray only",
                   "d_list_out == d_list_in or d_count_out == d_count_in when both are non-NULL",   # the aliasing rule
                   "exactly one of d_list_out and d_count_out given", "d_keep NULL", "a compaction with no output list",
                   "n_rays == 0: RT_OK", "n_rays > 0x7FFFFFFF: RT_ERR_UNSUPPORTED", "any RT_FLAG_MODE_*: RT_ERR_UNSUPPORTED",
                   "allowed while a progressive session is open", "no call reads the count on the host",
                   "RT_LIST_TILE (64 .. 65536, a power of two", "It changes no result",
                   "samples = ray_segments = the valid listed rays", "a compaction counts nothing",
                   "RT_KERNEL_LIST(kernel_id) is set"):
        assert phrase in doc, phrase


def test_the_list_bit_decodes_alike_in_c_and_python():
    text = open(HEADER).read()
    m = re.search(r"#define RT_KERNEL_LIST\(id\) \(\(\(id\) >> (\d+)\) & 1u\)", text)
    assert m and int(m.group(1)) == 18
    for kid in (0x8000 | 1 << 18, 0x8000 | 1 << 18 | 1 << 17 | 1 | 4 << 1, 0x8000 | 1 << 17 | 5 << 1, 0x808C, 0x81F9,
                0x8000 | 1 << 16, 0x8000 | 1 << 12 | 1 << 7):
        assert abi.RT_KERNEL_LIST(kid) == (kid >> 18) & 1 and abi.kernel_info(kid)["list"] == bool((kid >> 18) & 1)
    s = 0x8000 | 1 << 17 | 1 << 18
    assert abi.kernel_name(s | 1 | 4 << 1) == "path_step_list<double,false,false>"
    assert abi.kernel_name(s | 5 << 1 | 1 << 8 | 1 << 4) == "path_step_list<float,true,true>"
    only = abi.kernel_info(0x8000 | 1 << 18)
    assert only["list"] and not only["step"] and only["T"] == "float" and only["W"] == 0
    # existing ids decode unchanged
    assert abi.kernel_name(0x8000 | 1 << 17 | 1 | 4 << 1) == "path_step_rays<double,false,false>"
    assert abi.kernel_name(0x8000 | 1 << 16) == "scatter_rays<float>"
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"
    assert abi.kernel_name(0x81F9) == "trace_paths<double,4,true,3,true,true>"
    assert abi.kernel_name(0x8000 | 1 << 14 | 5 << 1 | 1 << 8) == "occlusion_rays<float,false,true>"
    assert not abi.kernel_info(0x808C)["list"] and abi.kernel_info(0) is None
    launch = open([f for f in abi.SOURCE_FILES if f.endswith("rt_launch.hpp")][0]).read()
    assert "kKernelListBit = 1u << 18" in launch


# ---------------------------------------------------------------- the entry points' refusals
def step(lib, ctx, n, li, ci, d_org, d_dir, d_col, d_pix, d_smp, bounce, flags, outs, lo, co):
    return lib.rt_path_step_list_async(ctx, n, li, ci, d_org, d_dir, d_col, d_pix, d_smp, bounce, 7, flags, *outs, lo, co, None)


def test_list_step_arguments_are_refused_without_a_gpu(lib):
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)   # never dereferenced: the checks come first
    ctx = ctypes.c_void_p(16)
    outs, none = (p, p, p, p, p), (None,) * 5
    invalid = [
        ("NULL ctx", (None, 64, p, p, p, p, p, p, p, 0, 0, outs, q, q)),
        ("NULL origins", (ctx, 64, p, p, None, p, p, p, p, 0, 0, outs, q, q)),
        ("NULL directions", (ctx, 64, None, None, p, None, p, p, p, 0, F32, outs, None, None)),
        ("NULL pixel", (ctx, 64, p, p, p, p, p, None, p, 0, 0, outs, q, q)),
        ("NULL sample", (ctx, 64, p, p, p, p, None, p, None, 0, 0, none, q, q)),
        ("list_out is list_in", (ctx, 64, p, p, p, p, p, p, p, 0, 0, outs, p, q)),
        ("count_out is count_in", (ctx, 64, p, p, p, p, p, p, p, 0, F32, outs, q, p)),
        ("list_out without count_out", (ctx, 64, p, p, p, p, p, p, p, 0, 0, outs, q, None)),
        ("count_out without list_out", (ctx, 64, None, None, p, p, p, p, p, 0, 0, outs, None, q)),
        ("unknown flag bits", (ctx, 64, p, p, p, p, p, p, p, 0, 0x40, outs, q, q)),
    ]
    for what, args in invalid:
        assert step(lib, *args) == abi.RT_ERR_INVALID, what
        assert STEP.encode() in lib.rt_last_error(), (what, lib.rt_last_error())
    for mode in (abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, abi.RT_FLAG_MODE_VECTORIZED3,
                 F32 | abi.RT_FLAG_ROOT2 | abi.RT_FLAG_MODE_VECTORIZED):
        assert step(lib, ctx, 64, p, p, p, p, p, p, p, 0, mode, outs, q, q) == abi.RT_ERR_UNSUPPORTED, mode
        assert STEP.encode() in lib.rt_last_error()
    assert step(lib, ctx, 64, p, p, p, p, p, p, p, abi.RT_MAX_BOUNCES_F32 + 1, F32, outs, q, q) == abi.RT_ERR_UNSUPPORTED
    assert STEP.encode() in lib.rt_last_error() and b"RT_MAX_BOUNCES_F32" in lib.rt_last_error()
    for flags in (0, F32, abi.RT_FLAG_ROOT2, F32 | abi.RT_FLAG_ROOT2):
        assert step(lib, ctx, 0x80000000, None, None, p, p, None, p, p, 1, flags, none, None, None) == abi.RT_ERR_UNSUPPORTED
        assert STEP.encode() in lib.rt_last_error() and b"too many rays" in lib.rt_last_error()


def test_compaction_arguments_are_refused_without_a_gpu(lib):
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)
    ctx = ctypes.c_void_p(16)
    invalid = [
        ("NULL ctx", (None, 64, p, p, p, q, q)),
        ("NULL keep", (ctx, 64, p, p, None, q, q)),
        ("no output list", (ctx, 64, p, p, p, None, None)),
        ("list_out without count_out", (ctx, 64, None, None, p, q, None)),
        ("count_out without list_out", (ctx, 64, p, p, p, None, q)),
        ("list_out is list_in", (ctx, 64, p, None, q, p, q)),
        ("count_out is count_in", (ctx, 64, None, p, q, q, p)),
    ]
    for what, args in invalid:
        assert lib.rt_ray_list_compact_async(*args, None) == abi.RT_ERR_INVALID, what
        assert COMPACT.encode() in lib.rt_last_error(), (what, lib.rt_last_error())
    assert lib.rt_ray_list_compact_async(ctx, 0x80000000, None, None, p, q, q, None) == abi.RT_ERR_UNSUPPORTED
    assert COMPACT.encode() in lib.rt_last_error() and b"too many rays" in lib.rt_last_error()


@pytest.mark.parametrize("name", [STEP, COMPACT])
def test_every_check_comes_before_any_device_work(name):
    """rt_context_create needs a device, so the GPU suite covers the no-scene refusal itself.  Here: the order of the
    checks in the source puts every one ahead of begin_launch, and the shared list check calls no HIP function."""
    src = open(abi.SOURCE_FILES[0]).read()
    body = src[src.index(f'extern "C" int {name}('):]
    body = body[:body.index("\n}\n")]
    assert body.index("NULL argument") < body.index("check_lists(") < body.index("n_rays == 0") < body.index("begin_launch")
    if name == STEP:
        assert body.index("check_lists(") < body.index("check_step(") < body.index("n_rays == 0")
    else:
        assert body.index("no output list") < body.index("too many rays") < body.index("n_rays == 0")
    shared = src[src.index("static int check_lists("):]
    shared = shared[:shared.index("\n}\n")]
    for text in ("given together", "d_list_out is d_list_in", "d_count_out is d_count_in"):
        assert text in shared, text
    assert "hip" not in shared


# ---------------------------------------------------------------- the renderer's own checks
def arrays(n=8, dtype=np.float32):
    d = FakeDevice(np.zeros((n, 3), dtype))
    o = FakeDevice(np.zeros((n, 3), dtype))
    u = FakeDevice(np.zeros(n, np.uint32))
    return o, d, u


def lists(n=8):
    return [FakeDevice(np.zeros(n, np.uint32)) for _ in range(2)], [FakeDevice(np.zeros(1, np.uint32)) for _ in range(2)]


@pytest.mark.parametrize("flags", [abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR, F32 | abi.RT_FLAG_MODE_VECTORIZED3])
def test_the_list_step_refuses_the_mode_renderers_before_touching_the_context(flags):
    o, d, u = arrays()
    with pytest.raises(ValueError, match="live path"):
        NoGpu(flags).path_step_list_into(o, d, u, u, bounce=0)


def test_the_into_methods_refuse_bad_arrays_before_any_gpu_call():
    r = NoGpu(F32, device=0)
    o, d, u = arrays()
    (la, lb), (ca, cb) = lists()
    k = FakeDevice(np.zeros(8, np.uint8))
    S = lambda **kw: r.path_step_list_into(o, d, u, u, bounce=0, **kw)   # noqa: E731
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        S(list_in=np.zeros(8, np.uint32))
    with pytest.raises(ValueError, match="dtype"):
        S(list_in=FakeDevice(np.zeros(8, np.int32)))
    with pytest.raises(ValueError, match="dtype"):
        S(list_out=la, count_out=FakeDevice(np.zeros(1, np.uint64)))
    with pytest.raises(ValueError, match="shape"):
        S(list_in=FakeDevice(np.zeros(7, np.uint32)))
    with pytest.raises(ValueError, match="shape"):
        S(count_in=FakeDevice(np.zeros(2, np.uint32)))
    with pytest.raises(ValueError, match="shape"):
        S(count_in=FakeDevice(np.zeros((), np.uint32)))
    with pytest.raises(ValueError, match="contiguous"):
        S(list_in=FakeDevice(np.zeros(16, np.uint32)[::2]))
    with pytest.raises(ValueError, match="read-only"):
        S(list_out=FakeDevice(np.zeros(8, np.uint32), readonly=True), count_out=ca)
    with pytest.raises(ValueError, match="read-only"):
        S(list_out=la, count_out=FakeDevice(np.zeros(1, np.uint32), readonly=True))
    with pytest.raises(ValueError, match="device"):
        S(list_in=FakeDevice(np.zeros(8, np.uint32), device=Dev("cuda", 1)))
    with pytest.raises(ValueError, match="dtype"):   # the step's own checks still run
        S(status=FakeDevice(np.zeros(8, np.int8)))
    with pytest.raises(TypeError, match="bounce"):   # keyword-only and required
        r.path_step_list_into(o, d, u, u)
    with pytest.raises(ValueError, match="dtype"):
        r.compact_list_into(FakeDevice(np.zeros(8, np.int8)), la, ca)
    with pytest.raises(ValueError, match="shape"):
        r.compact_list_into(k, FakeDevice(np.zeros(9, np.uint32)), ca)
    r.seed = 1
    r._scene_flat = None
    with pytest.raises(TypeError, match="stream"):
        S(stream="0")
    with pytest.raises(TypeError, match="stream"):
        r.compact_list_into(k, la, ca, stream=1.5)
    with pytest.raises(RuntimeError, match="path_step_list_into needs a scene"):
        S(list_in=la, count_in=ca, list_out=lb, count_out=cb)
    # what the checks hand on
    got = checks.check_path_step_list_into(F32, 0, o, d, u, u, None, dict(status=None, index=None, t=None, normal=None, front=None),
                                           3, la, ca, lb, cb)
    assert got[0] == 8 and got[1] == o.a.ctypes.data and got[6] == {} and got[7] == 3
    assert got[8] == (la.a.ctypes.data, ca.a.ctypes.data, lb.a.ctypes.data, cb.a.ctypes.data)
    assert checks.check_lists(0, 8, None, None, None, None) == (None, None, None, None)
    n, d_keep, ptrs = checks.check_compact_list_into(0, k, la, ca, None, None)
    assert n == 8 and d_keep == k.a.ctypes.data and ptrs == (None, None, la.a.ctypes.data, ca.a.ctypes.data)


class Huge:
    """A device array's description alone: (2^31,) uint8, never allocated."""
    __cuda_array_interface__ = {"shape": (1 << 31,), "typestr": "|u1", "data": (16, False), "version": 3}


def test_every_raise_of_the_list_checks_is_reached_and_worded():
    """tests/test_renderer_messages.py's bar for the new module: each raise statement of list_checks.py is the end of a
    call below, and its type and full text are pinned."""
    r = NoGpu(F32, device=0)
    o, d, u = arrays()
    (la, lb), (ca, cb) = lists()
    k = FakeDevice(np.zeros(8, np.uint8))
    S = lambda **kw: r.path_step_list_into(o, d, u, u, bounce=0, **kw)   # noqa: E731
    cases = [
        (lambda: S(list_out=la), ValueError, "list_out and count_out must be given together (or neither: no output list)"),
        (lambda: r.compact_list_into(k, None, None), ValueError, "a compaction needs an output list: list_out and count_out"),
        (lambda: S(list_in=la, list_out=la, count_out=ca), ValueError, "list_out is list_in: ping-pong two lists"),
        (lambda: r.compact_list_into(k, la, ca, count_in=ca), ValueError, "count_out is count_in: ping-pong two counts"),
        (lambda: r.compact_list_into(np.zeros(8, np.uint8), la, ca), TypeError,
         "keep must be a device array of shape (n,), one uint8 per ray id"),
        (lambda: r.compact_list_into(Huge(), la, ca), ValueError, "more than 0x7FFFFFFF rays in one list"),
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


def test_path_trace_takes_compact_and_leaves_the_default_loop_alone():
    import inspect
    from rt_mi355x import integrators
    sig = inspect.signature(integrators.path_trace)
    assert sig.parameters["compact"].default is False
    assert "compact" not in inspect.signature(integrators.direct_light).parameters
    stats = {}
    out = integrators.path_trace(NoGpu(F32), np.zeros((0, 3)), np.zeros((0, 3)), None, None, 4, None, stats=stats, compact=True)
    assert out.shape == (0, 3) and out.dtype == np.float32 and stats["steps"] == 0 and stats["invalid"] == 0
