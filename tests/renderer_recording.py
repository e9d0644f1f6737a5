"""A recording stand-in for the HIP library, and the calls that tests/test_renderer_calls.py and
tests/test_renderer_messages.py replay through rt_mi355x.renderer's public API.

FakeLib is a plain Python object: every rt_* attribute logs its name and arguments and returns RT_OK, so
GpuRenderer(lib=FakeLib()) runs without the built library and without a GPU.  CALL_CASES maps a name to a function
of a fresh FakeLib that drives the renderer; FAILURE_CASES are the six methods that make a device round trip;
MESSAGE_CASES each raise from an argument check.  tests/golden/make_renderer_golden.py records what they give.
"""
import ast
import ctypes
import os
import traceback

import numpy as np

import rt_mi355x as rt
from rt_mi355x import abi

DEVICE_BASE = 0x7D0000000000    # fake device pointers: no integer argument of a call comes near these
CONTEXT_BASE = 0x7C0000000000
CALLER_BASE = 0x7E0000000000    # device arrays of the caller's own (DeviceArray): slot k is at CALLER_BASE + 0x1000 k
HOST_ADDRESS = {("rt_memcpy_d2h", 1), ("rt_memcpy_h2d", 2)}   # (call, argument) that is an integer host address
STRUCT_INPUTS = (abi.RtCamera, abi.RtTileRange)


class FakeLib:
    """Logs every call as [name, argument...]: integers and floats as they are, None (and a NULL c_void_p) as null,
    RtCamera / RtTileRange by field values, RtScene by its two counts, a device pointer as {"dev": index of the
    allocation}, a caller's device array as {"caller": slot}, the context as "ctx", a host address as "host", any other byref as "out".
    fail_at: the index in `calls` of the call that returns RT_ERR_HIP instead of doing its work."""

    def __init__(self, refine_active=(1,), items=0, collect_rc=abi.RT_OK):
        self.calls, self.handed, self.freed, self.contexts = [], [], [], []
        self.fail_at = None
        self.refine_active, self.items, self.collect_rc = list(refine_active), items, collect_rc

    def __getattr__(self, name):
        if not name.startswith("rt_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        k = len(self.calls)
        self.calls.append([name] + [self._log(name, i, a) for i, a in enumerate(args)])
        if name == "rt_last_error":
            return b"injected failure"
        if k == self.fail_at:
            return abi.RT_ERR_HIP
        handler = getattr(self, "_" + name, None)
        return handler(*args) if handler else abi.RT_OK

    def _log(self, name, i, a):
        if a is None:
            return None
        if isinstance(a, ctypes.c_void_p):
            a = a.value
            if a is None:
                return None
        if isinstance(a, (int, np.integer)) and not isinstance(a, bool):
            a = int(a)
            if (name, i) in HOST_ADDRESS:
                return "host"
            if a in self.contexts:
                return "ctx"
            if a in self.handed:
                return {"dev": self.handed.index(a)}
            if a >= CALLER_BASE:
                return {"caller": (a - CALLER_BASE) // 0x1000}
            return a
        if isinstance(a, float):
            return a
        if isinstance(a, (ctypes._Pointer, ctypes.Array)):
            return "host"
        obj = getattr(a, "_obj", None)   # byref(obj)
        if isinstance(obj, abi.RtScene):
            return {"n_spheres": obj.n_spheres, "n_materials": obj.n_materials}
        if isinstance(obj, STRUCT_INPUTS):
            return {f: (v if isinstance(v, int) else list(v)) for f, v in ((f, getattr(obj, f)) for f, _ in obj._fields_)}
        if obj is not None:
            return "out"
        raise TypeError(f"{name}: argument {i} is {a!r}")

    # what the calls with outputs write
    def _rt_context_create(self, device, ref):
        self.contexts.append(CONTEXT_BASE + 0x1000 * len(self.contexts))
        ref._obj.value = self.contexts[-1]
        return abi.RT_OK

    def _rt_device_alloc(self, ctx, nbytes, ref):
        self.handed.append(DEVICE_BASE + 0x1000 * len(self.handed))
        ref._obj.value = self.handed[-1]
        return abi.RT_OK

    def _rt_device_free(self, ctx, ptr):
        self.freed.append(ptr.value if isinstance(ptr, ctypes.c_void_p) else ptr)
        return abi.RT_OK

    def _rt_memcpy_d2h(self, ctx, dst, src, nbytes):
        ctypes.memset(dst, 0, nbytes)   # dst is a numpy array of nbytes: the read-back is zeros
        return abi.RT_OK

    def _rt_context_collect(self, ctx, stream, ref):
        st = ref._obj
        st.kernel_ms, st.samples, st.ray_segments, st.bounce_iters = 1.5, 7, 11, 13
        return self.collect_rc

    def _rt_progressive_refine(self, ctx, tolerance, spp_max, stream, n_active, n_samples):
        n = self.refine_active.pop(0) if self.refine_active else 0
        n_active._obj.value, n_samples._obj.value = n, 3 * n
        return abi.RT_OK

    def _rt_progressive_refine_items(self, ctx, per_item, n, items, capacity):
        per_item._obj.value, n._obj.value = (4 if self.items else 0), self.items
        return abi.RT_OK


def describe(x):
    """A returned value as JSON: shapes and dtypes of arrays (their memory is the fake's), the fields of the stats."""
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.ndarray):
        return {"ndarray": x.dtype.name, "shape": list(x.shape)}
    if isinstance(x, abi.RtStats):
        return {"RtStats": [x.kernel_ms, x.samples, x.ray_segments, x.bounce_iters]}
    if isinstance(x, rt.RenderStat):
        return {"RenderStat": [x.pixels_rendered(), x.kernel_ms, x.samples, x.ray_segments, x.range_error, x.bounce_iters]}
    if isinstance(x, dict):
        return {k: describe(v) for k, v in x.items()}
    if isinstance(x, tuple) and hasattr(x, "_fields"):
        return {type(x).__name__: [describe(v) for v in x]}
    if isinstance(x, (tuple, list)):
        return [describe(v) for v in x]
    raise TypeError(f"cannot describe {x!r}")


# ---------------------------------------------------------------- the shapes: 10 spheres, 8x4 pixels, 5 rays
SCENE = rt.scenes.random_spheres(10)
FLAT = SCENE.flatten()
OTHER = rt.scenes.three_spheres().flatten()
CAM = rt.camera_new_py(8, 4, **rt.MAIN_CAMERA)
CAMERA = rt.Camera.from_abi(CAM)
TILE = abi.RtTileRange(1, 2, 2, 3, 4)
N = 5
DIRS = np.arange(N * 3, dtype=np.float64).reshape(N, 3) + 1.0
DIRS2 = np.arange(N * 2 * 3, dtype=np.float64).reshape(N, 2, 3) + 1.0
ORIGIN = np.array([16.0, 2.0, 18.5])
STREAM = 0x5EED


class Dev:
    def __init__(self, type_, index):
        self.type, self.index = type_, index

    def __str__(self):
        return f"{self.type}:{self.index}"


class DeviceArray:
    """An object exposing __cuda_array_interface__ with the shape, dtype and strides of a numpy array, as a torch
    ROCm tensor does.  Its pointer is a made-up one (the checks never dereference it), the same in every run."""

    def __init__(self, a, readonly=False, device=None, null=False, slot=0):
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": a.dtype.str, "version": 3,
                                         "data": (0 if null else CALLER_BASE + 0x1000 * slot, readonly),
                                         "strides": None if a.flags.c_contiguous else a.strides}
        if device is not None:
            self.device = device


class ShapeOnly:
    """Claims a shape without the memory: for the checks on counts above 2^31."""

    def __init__(self, shape, dtype=np.float64):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": np.dtype(dtype).str, "version": 3,
                                         "data": (1 << 20, False), "strides": None}


def dev(shape, dtype=np.float64, **kw):
    return DeviceArray(np.zeros(shape, dtype), **kw)


def renderer(fake, **kw):
    return rt.GpuRenderer(lib=fake, **kw)


# ---------------------------------------------------------------- calls to replay
def _second_render(fake):
    r = renderer(fake)
    r.render_flat(8, 3, FLAT, CAM)
    n = len(fake.calls)
    r.render_flat(8, 3, FLAT, CAM)                       # the same FlatScene: no rt_context_set_scene
    same = [c[0] for c in fake.calls[n:]]
    r.render_flat(8, 3, OTHER, CAM)                      # another: one
    return r, ("rt_context_set_scene" in same, r._scene_flat is OTHER)


def _query(fake, origins, **kw):
    r = renderer(fake, **{k: kw.pop(k) for k in ("precision",) if k in kw})
    out = r.query(origins, kw.pop("directions", DIRS), FLAT, **kw)
    return r, (out, r.query_stats)


def _query_into(fake, origins, precision="f64", **outputs):
    r = renderer(fake, precision=precision)
    r.set_scene(FLAT)
    return r, r.query_into(origins, dev((N, 3), np.float32 if precision == "f32" else np.float64, slot=9),
                           stream=STREAM, **outputs)


def _rays_into(fake, origins, directions, **kw):
    r = renderer(fake)
    r.set_scene(FLAT)
    return r, r.render_rays_into(8, 4, origins, directions, stream=STREAM, **kw)


def _session(fake):
    r = renderer(fake)
    out = []
    s = r.begin_progressive(8, 16, SCENE, CAMERA)
    out.append((r._session is s, s.npx, s.capacity))
    out.append(s.extend(2))
    out.append(s.extend(3, want_linear=True, stream=STREAM))
    out.append(s.extend(4, image=False))
    out.append(s.extend_map(np.full(32, 5, dtype=np.int64), want_linear=True))
    out.append(s.extend_map(np.full(32, 6, dtype=np.uint32), image=False))
    out.append(s.snapshot())
    out.append(s.snapshot(np.full(32, 2), want_linear=True))
    out.append(s.error())
    out.append(s.error(stats=True, stream=STREAM))
    out.append(s.refine(0.25, 16))
    out.append(s.refine_items())
    out.append(s.collect())
    out.append(s.counts)     # stale after the refine: one rt_progressive_counts
    out.append(s.done)       # fresh: none
    out.append(s.refine(0.25, 16, stream=STREAM))
    out.append(s.done)
    out.append(s.collect(stream=STREAM))
    s.close()
    out.append((r._session is None, s._open))
    s.close()                # a second close makes no call
    for closed in (lambda: s.extend(5), lambda: s.snapshot(), lambda: s.error(), lambda: s.refine(0.5, 16),
                   lambda: s.refine_items()):
        try:
            closed()
        except RuntimeError as e:
            out.append(str(e))
    out.append(s.counts)     # the counts last read
    return r, out


def _session_tile(fake):
    r = renderer(fake, precision="f32")
    with r.begin_progressive(8, 16, FLAT, CAM, tile_range=TILE, max_bytes=1 << 20) as s:
        out = [s.npx, s.extend(2, want_linear=True), s.refine(0.5, 8), s.refine_items()]
    return r, out


def _close_with_session(fake):
    r = renderer(fake)
    s = r.begin_progressive(8, 4, FLAT, CAM)
    r.close()
    state = (s._open, r._session is None, bool(r.ctx))
    s.close()
    r.close()    # neither makes a call
    return r, state


def _failed_upload(fake):
    r = renderer(fake)
    r.set_scene(FLAT)
    fake.fail_at = len(fake.calls)
    try:
        r.set_scene(OTHER)
    except rt.RtError as e:
        return r, (str(e), e.code, r._scene_flat is None)


def _with(fn, **fake_kw):
    """The case fn, run over FakeLib(**fake_kw)."""
    def case(fake):
        return fn(fake)
    case.fake_kw = fake_kw
    return case


def _progressive(schedule, scene, camera):
    def case(fake):
        r = renderer(fake)
        return r, list(r.progressive(8, schedule, scene, camera))
    return case


def _r(method, *args, **kw):
    """A case: method(*args) of a fresh renderer (renderer keywords under `new`)."""
    new = kw.pop("new", {})

    def case(fake):
        r = renderer(fake, **new)
        return r, getattr(r, method)(*args, **kw)
    return case


RANGE = dict(collect_rc=abi.RT_ERR_RANGE)
CALL_CASES = {
    "render_flat": _r("render_flat", 8, 3, FLAT, CAM),
    "render_flat_linear": _r("render_flat", 8, 3, FLAT, CAM, want_linear=True),
    "render_flat_split_plan": _r("render_flat", 8, 3, FLAT, CAM, samples_per_item=0),
    "render_flat_split_3_linear": _r("render_flat", 8, 6, FLAT, CAM, want_linear=True, samples_per_item=3),
    "render_flat_tile": _r("render_flat", 8, 3, FLAT, CAM, tile_range=TILE, want_linear=True, new=dict(precision="f32")),
    "render_flat_range": _with(_r("render_flat", 8, 1, FLAT, CAM), **RANGE),
    "render": _r("render", 8, 3, SCENE, CAMERA),
    "render_flat_arguments": _r("render", 8, 3, FLAT, CAM, new=dict(mode="scalar", root2=True, seed=7, device=1)),
    "render_sample_parallel": _r("render", 8, 3, SCENE, CAMERA, new=dict(sample_parallel=True)),
    "render_range": _with(_r("render", 8, 1, SCENE, CAMERA), **RANGE),
    "second_render": _second_render,
    "failed_upload": _failed_upload,
    "guides_flat": _r("guides_flat", 3, FLAT, CAM),
    "guides_flat_depth_albedo": _r("guides_flat", 3, FLAT, CAM, tile_range=TILE, want=("depth", "albedo")),
    "guides": _r("guides", 3, SCENE, CAMERA, new=dict(precision="f32")),
    "query_shared": lambda fake: _query(fake, ORIGIN),
    "query_per_ray": lambda fake: _query(fake, DIRS[::-1]),
    "query_subset_f32": lambda fake: _query(fake, ORIGIN, want=("index", "t"), precision="f32"),
    "query_empty": lambda fake: _query(fake, ORIGIN, directions=np.zeros((0, 3))),
    "query_root2": lambda fake: _query(fake, DIRS, root2=True, want=("front",)),
    "query_into_shared": lambda fake: _query_into(fake, ORIGIN, t=dev(N, slot=1), front=dev(N, np.uint8, slot=5)),
    "query_into_device_f32": lambda fake: _query_into(fake, dev((N, 3), np.float32, slot=8), "f32",
                                                      index=dev(N, np.int32, slot=2), normal=dev((N, 3), np.float32, slot=3),
                                                      point=dev((N, 3), np.float32, slot=4)),
    "render_rays": _r("render_rays", 8, 4, ORIGIN, DIRS, FLAT),
    "render_rays_per_ray_linear": _r("render_rays", 8, 4, DIRS2[::-1], DIRS2, SCENE, want_linear=True),
    "render_rays_shared_R2_f32": _r("render_rays", 8, 4, ORIGIN, DIRS2, FLAT, want_linear=True, root2=True,
                                    new=dict(precision="f32")),
    "render_rays_empty": _r("render_rays", 8, 4, ORIGIN, np.zeros((0, 3)), FLAT, want_linear=True),
    "render_rays_seed_base": _r("render_rays", 8, 4, DIRS, DIRS, FLAT, seed=99, pixel_base=(1 << 32) - N),
    "render_rays_range": _with(_r("render_rays", 8, 4, ORIGIN, DIRS, FLAT), **RANGE),
    "render_rays_into_shared": lambda fake: _rays_into(fake, ORIGIN, dev((N, 3), slot=9), rgb=dev((N, 3), np.uint8, slot=1)),
    "render_rays_into_device": lambda fake: _rays_into(fake, dev((N, 2, 3), slot=8), dev((N, 2, 3), slot=9),
                                                       linear=dev((N, 3), slot=2), rgb=dev((N, 3), np.uint8, slot=1),
                                                       seed=99, pixel_base=64, root2=True),
    "session": _session,
    "session_items": _with(_session_tile, items=2),
    "session_range": _with(_session_tile, **RANGE),
    "progressive": _progressive([1, 2, 4], SCENE, CAMERA),
    "progressive_range": _with(_progressive((2, 3), FLAT, CAM), **RANGE),
    "adaptive_host": _r("adaptive", 8, 2, 16, 0.01, SCENE, CAMERA),
    "adaptive_device": _r("adaptive", 8, 2, 16, 0.01, FLAT, CAM, plan="device"),
    "adaptive_device_two_steps": _with(_r("adaptive", 8, 2, 16, 0.01, FLAT, CAM, plan="device"), refine_active=(3, 1)),
    "adaptive_range": _with(_r("adaptive", 8, 2, 16, 0.01, FLAT, CAM), **RANGE),
    "close_with_session": _close_with_session,
}


def run_case(case):
    """(fake, what the case returned or raised, described) with a fresh FakeLib; the renderer is closed afterwards,
    outside the record."""
    fake = FakeLib(**getattr(case, "fake_kw", {}))
    r = None
    try:
        r, result = case(fake)
        result = describe(result)
    except Exception as e:
        result = {"raises": type(e).__name__, "text": str(e)}
    calls = list(fake.calls)
    if r is not None:
        r.close()
    return fake, {"calls": calls, "result": result}


# ---------------------------------------------------------------- the six round trips, for the failure sweep
def _later(method, *args, session=False, **kw):
    """setup(fake) -> the call to make, on a fresh renderer or on a session opened on one (the calls the setup itself
    makes are not part of the sweep)."""
    def setup(fake):
        obj = renderer(fake)
        if session:
            obj = obj.begin_progressive(8, 16, FLAT, CAM)
        return lambda: getattr(obj, method)(*args, **kw)
    return setup


FAILURE_CASES = {
    "render_flat": _later("render_flat", 8, 3, FLAT, CAM, want_linear=True),
    "render_flat_split": _later("render_flat", 8, 3, FLAT, CAM, samples_per_item=0),
    "guides_flat": _later("guides_flat", 3, FLAT, CAM),
    "query": _later("query", DIRS, DIRS, FLAT),
    "query_shared": _later("query", ORIGIN, DIRS, FLAT, want=("t",)),
    "render_rays": _later("render_rays", 8, 4, DIRS2, DIRS2, FLAT, want_linear=True),
    "render_rays_shared": _later("render_rays", 8, 4, ORIGIN, DIRS, FLAT),
    "session.extend": _later("extend", 2, want_linear=True, session=True),
    "session.extend_no_image": _later("extend", 2, image=False, session=True),
    "session.error": _later("error", stats=True, session=True),
}


# ---------------------------------------------------------------- every raise an argument check can reach
class NoLibrary(rt.GpuRenderer):
    """A renderer without library or context: a check that came after their first use would raise AttributeError."""

    def __init__(self, flags=0, device=0):
        self.flags, self.device = flags, device

    def __del__(self):
        pass


def _messages():
    f32, scalar = abi.RT_FLAG_F32, abi.RT_FLAG_MODE_SCALAR
    r, bad = NoLibrary(f32), NoLibrary(scalar)
    lib_r = rt.GpuRenderer(lib=FakeLib())   # render_flat binds the library before it checks
    d32 = dev((N, 3), np.float32)
    d32r = dev((N, 2, 3), np.float32)
    t32 = dict(t=dev(N, np.float32))
    rgb = dict(rgb=dev((N, 3), np.uint8))
    huge = np.broadcast_to(np.zeros(3), (1 << 31, 3))
    cases = {
        "Renderer.render": lambda: rt.Renderer().render(8, 4, None, None),
        "mode": lambda: rt.GpuRenderer(mode="vectorised", lib=FakeLib()),
        "precision": lambda: rt.GpuRenderer(precision="f16", lib=FakeLib()),
        "split type": lambda: lib_r.render_flat(8, 4, FLAT, CAM, samples_per_item=True),
        "split type float": lambda: lib_r.render_flat(8, 4, FLAT, CAM, samples_per_item=2.0),
        "split type numpy": lambda: lib_r.render_flat(8, 4, FLAT, CAM, samples_per_item=np.int64(2)),
        "split negative": lambda: lib_r.render_flat(8, 4, FLAT, CAM, samples_per_item=-1),
        "schedule empty": lambda: r.progressive(8, [], SCENE, CAMERA),
        "schedule entry": lambda: r.progressive(8, [1, 2.0], SCENE, CAMERA),
        "schedule bool": lambda: r.progressive(8, [True, 2], SCENE, CAMERA),
        "schedule start": lambda: r.progressive(8, [0, 2], SCENE, CAMERA),
        "schedule order": lambda: r.progressive(8, [1, 4, np.int32(4)], SCENE, CAMERA),
        "adaptive plan": lambda: r.adaptive(8, 1, 4, 0.1, SCENE, CAMERA, plan="gpu"),
        "adaptive int": lambda: r.adaptive(8, 1.0, 4, 0.1, SCENE, CAMERA),
        "adaptive int max": lambda: r.adaptive(8, 1, True, 0.1, SCENE, CAMERA, plan="device"),
        "adaptive min": lambda: r.adaptive(8, 0, 4, 0.1, SCENE, CAMERA),
        "adaptive order": lambda: r.adaptive(8, 5, np.int64(4), 0.1, SCENE, CAMERA),
        "adaptive nan": lambda: r.adaptive(8, 1, 4, float("nan"), SCENE, CAMERA),
        "guides mode": lambda: bad.guides(4, SCENE, CAMERA),
        "guides root2": lambda: NoLibrary(abi.RT_FLAG_ROOT2).guides_flat(4, FLAT, CAM),
        "guides name": lambda: r.guides_flat(4, FLAT, CAM, want=("depth", "colour")),
        "guides none": lambda: r.guides_flat(4, FLAT, CAM, want=()),
        # query
        "query mode": lambda: bad.query(ORIGIN, DIRS, None),
        "query name": lambda: r.query(ORIGIN, DIRS, None, want=("t", "uv")),
        "query none": lambda: r.query(ORIGIN, DIRS, None, want=[]),
        "query directions dtype": lambda: r.query(ORIGIN, DIRS.astype(complex), None),
        "query origins dtype": lambda: r.query(np.array(["a", "b", "c"]), DIRS, None),
        "query directions shape": lambda: r.query(ORIGIN, DIRS2, None),
        "query origins shape": lambda: r.query(DIRS[:4], DIRS, None),
        "query count": lambda: r.query(ORIGIN, huge, None),
        # query_into
        "query_into mode": lambda: bad.query_into(ORIGIN, d32, **t32),
        "query_into host directions": lambda: r.query_into(ORIGIN, DIRS, **t32),
        "query_into directions shape": lambda: r.query_into(ORIGIN, d32r, **t32),
        "query_into count": lambda: r.query_into(ORIGIN, ShapeOnly((1 << 31, 3), np.float32), **t32),
        "query_into directions dtype": lambda: r.query_into(ORIGIN, dev((N, 3)), **t32),
        "query_into origins shape": lambda: r.query_into(dev((4, 3), np.float32), d32, **t32),
        "query_into shared origin": lambda: r.query_into(np.zeros(2), d32, **t32),
        "query_into shared origin dtype": lambda: r.query_into(np.zeros(3, complex), d32, **t32),
        "query_into strides": lambda: r.query_into(ORIGIN, DeviceArray(np.zeros((N, 6), np.float32)[:, ::2]), **t32),
        "query_into device": lambda: r.query_into(ORIGIN, dev((N, 3), np.float32, device=Dev("cuda", 1)), **t32),
        "query_into device kind": lambda: r.query_into(ORIGIN, d32, t=dev(N, np.float32, device=Dev("cpu", None))),
        "query_into null": lambda: r.query_into(ORIGIN, d32, t=dev(N, np.float32, null=True)),
        "query_into host output": lambda: r.query_into(ORIGIN, d32, t=np.zeros(N, np.float32)),
        "query_into output dtype": lambda: r.query_into(ORIGIN, d32, index=dev(N, np.int64)),
        "query_into output shape": lambda: r.query_into(ORIGIN, d32, normal=dev(N, np.float32)),
        "query_into read-only": lambda: r.query_into(ORIGIN, d32, front=dev(N, np.uint8, readonly=True)),
        "query_into none": lambda: r.query_into(ORIGIN, d32),
        "query_into stream": lambda: r.query_into(ORIGIN, d32, stream="0", **t32),
        "query_into stream bool": lambda: r.query_into(ORIGIN, d32, stream=True, **t32),
        "query_into stream numpy": lambda: r.query_into(ORIGIN, d32, stream=np.int64(0), **t32),
        "query_into scene": lambda: rt.GpuRenderer(lib=FakeLib(), precision="f32").query_into(ORIGIN, d32, **t32),
        # render_rays
        "render_rays mode": lambda: bad.render_rays(8, 4, ORIGIN, DIRS, None),
        "render_rays directions dtype": lambda: r.render_rays(8, 4, ORIGIN, DIRS.astype(complex), None),
        "render_rays origins dtype": lambda: r.render_rays(8, 4, np.array([None, None, None]), DIRS, None),
        "render_rays directions shape": lambda: r.render_rays(8, 4, ORIGIN, np.zeros((N, 2)), None),
        "render_rays directions rank": lambda: r.render_rays(8, 4, ORIGIN, np.zeros((2, N, 3, 3)), None),
        "render_rays origins shape": lambda: r.render_rays(8, 4, DIRS, DIRS2, None),
        "render_rays spp": lambda: r.render_rays(8, 0, ORIGIN, DIRS, None),
        "render_rays spp bool": lambda: r.render_rays(8, True, ORIGIN, DIRS, None),
        "render_rays spp float": lambda: r.render_rays(8, 2.5, ORIGIN, DIRS, None),
        "render_rays spp large": lambda: r.render_rays(8, (1 << 20) + 1, ORIGIN, DIRS, None),
        "render_rays rays per pixel": lambda: r.render_rays(8, 1, ORIGIN, DIRS2, None),
        "render_rays count": lambda: r.render_rays(8, 4, ORIGIN, huge, None),
        "render_rays pixel_base": lambda: r.render_rays(8, 4, ORIGIN, DIRS, None, pixel_base=-1),
        "render_rays pixel_base end": lambda: r.render_rays(8, 4, ORIGIN, DIRS, None, pixel_base=(1 << 32) - N + 1),
        "render_rays pixel_base float": lambda: r.render_rays(8, 4, ORIGIN, DIRS, None, pixel_base=1.5),
        # render_rays_into
        "render_rays_into mode": lambda: bad.render_rays_into(8, 4, ORIGIN, d32, **rgb),
        "render_rays_into host directions": lambda: r.render_rays_into(8, 4, ORIGIN, DIRS, **rgb),
        "render_rays_into directions shape": lambda: r.render_rays_into(8, 4, ORIGIN, dev((N, 2, 4), np.float32), **rgb),
        "render_rays_into directions rank": lambda: r.render_rays_into(8, 4, ORIGIN, dev(3, np.float32), **rgb),
        "render_rays_into spp": lambda: r.render_rays_into(8, np.int64(0), ORIGIN, d32, **rgb),
        "render_rays_into rays per pixel": lambda: r.render_rays_into(8, 1, ORIGIN, d32r, **rgb),
        "render_rays_into count": lambda: r.render_rays_into(8, 4, ORIGIN, ShapeOnly((1 << 31, 3), np.float32), **rgb),
        "render_rays_into pixel_base": lambda: r.render_rays_into(8, 4, ORIGIN, d32, pixel_base=1 << 32, **rgb),
        "render_rays_into directions dtype": lambda: r.render_rays_into(8, 4, ORIGIN, dev((N, 3)), **rgb),
        "render_rays_into origins shape": lambda: r.render_rays_into(8, 4, d32, d32r, **rgb),
        "render_rays_into shared origin": lambda: r.render_rays_into(8, 4, np.zeros(4), d32r, **rgb),
        "render_rays_into strides": lambda: r.render_rays_into(
            8, 4, ORIGIN, d32, rgb=DeviceArray(np.zeros((2 * N, 3), np.uint8)[::2])),
        "render_rays_into host output": lambda: r.render_rays_into(8, 4, ORIGIN, d32, rgb=np.zeros((N, 3), np.uint8)),
        "render_rays_into output dtype": lambda: r.render_rays_into(8, 4, ORIGIN, d32, linear=dev((N, 3), np.float32)),
        "render_rays_into output shape": lambda: r.render_rays_into(8, 4, ORIGIN, d32r, linear=dev((N, 2, 3))),
        "render_rays_into read-only": lambda: r.render_rays_into(8, 4, ORIGIN, d32, linear=dev((N, 3), readonly=True)),
        "render_rays_into device": lambda: r.render_rays_into(8, 4, ORIGIN, d32, rgb=dev((N, 3), np.uint8, device=Dev("cuda", 3))),
        "render_rays_into none": lambda: r.render_rays_into(8, 4, ORIGIN, d32),
        "render_rays_into stream": lambda: r.render_rays_into(8, 4, ORIGIN, d32, stream=1.0, **rgb),
        "render_rays_into stream bool": lambda: r.render_rays_into(8, 4, ORIGIN, d32, stream=False, **rgb),
        "render_rays_into scene": lambda: rt.GpuRenderer(lib=FakeLib(), precision="f32").render_rays_into(
            8, 4, ORIGIN, d32, **rgb),
    }
    # a session's per-pixel maps (the session itself is open on the recording library)
    s = rt.GpuRenderer(lib=FakeLib()).begin_progressive(8, 16, FLAT, CAM)
    cases.update({
        "targets length": lambda: s.extend_map(np.zeros(31, np.uint32)),
        "targets dtype": lambda: s.extend_map(np.zeros(32)),
        "targets negative": lambda: s.extend_map(np.full(32, -1)),
        "targets large": lambda: s.extend_map(np.full(32, 1 << 32)),
        "counts shape": lambda: s.snapshot(np.zeros((4, 8), np.uint32)),
    })
    return cases


MESSAGE_CASES = _messages()

PACKAGE = os.path.dirname(os.path.abspath(rt.__file__))
CHECKED_SOURCES = [f for f in ("renderer.py", "checks.py", "session.py") if os.path.exists(os.path.join(PACKAGE, f))]


def run_message(call):
    """(exception type name, text, (file, line) of the raise within CHECKED_SOURCES or None)."""
    try:
        call()
    except Exception as e:
        where = None
        for frame in traceback.extract_tb(e.__traceback__):
            if os.path.dirname(frame.filename) == PACKAGE and os.path.basename(frame.filename) in CHECKED_SOURCES:
                where = (os.path.basename(frame.filename), frame.lineno)
        return type(e).__name__, str(e), where
    raise AssertionError("the call raised nothing")


def raise_statements():
    """{(file, first line): source text} of every raise statement in CHECKED_SOURCES, and for each the lines it spans."""
    found = {}
    for f in CHECKED_SOURCES:
        text = open(os.path.join(PACKAGE, f)).read()
        for node in ast.walk(ast.parse(text)):
            if isinstance(node, ast.Raise):
                found[(f, node.lineno)] = (ast.get_source_segment(text, node), range(node.lineno, node.end_lineno + 1))
    return found


def unreached_raises():
    """The source text of the raise statements no MESSAGE_CASES call ends at."""
    hit = {run_message(call)[2] for call in MESSAGE_CASES.values()}
    return sorted(text for (f, _), (text, lines) in raise_statements().items()
                  if not any(h is not None and h[0] == f and h[1] in lines for h in hit))


def allowed_unreached(text):
    """What the message cases may leave out (test_renderer_calls.py covers it): the two RT_ERR_RANGE raises, which
    need a collect that reports the code, and the calls on a closed session."""
    return "a pixel channel exceeded 2.0" in text or "the progressive session is closed" in text
