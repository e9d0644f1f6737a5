"""Renderer trait mirror (src/renderer.rs:11-40) backed by the MI355X C ABI.

    trait Renderer { fn render(&self, max_bounces, samples_per_pixel, &Arc<Scene>, &Arc<Camera>)
                     -> (RgbImage, RenderStat) }                       renderer.rs:38-40
    TileRenderer::new(num_threads: Option<NonZeroUsize>, block_size)   renderer.rs:232-241

`GpuRenderer.render` has the same argument meaning and returns (image HxWx3 uint8 numpy array,
RenderStat).  Where the reference panics (Color::to_u8_array's `<= 2.0` assert,
color.rs:55-57; unknown material, materials.rs:31; spp == 0 -> 0/0) this raises RtError.
There is no CPU fallback: the HIP library must be built and a GPU present.
"""
import collections
import ctypes
import time

import numpy as np

from . import abi


class RenderStat:
    """renderer.rs:11-34 (+ the GPU work counters)."""

    def __init__(self, duration, pixels_rendered, kernel_ms=0.0, samples=0, ray_segments=0, range_error=False,
                 bounce_iters=0):
        # range_error (GpuRenderer.progressive only): a pixel channel exceeded 2.0 at this step (RT_ERR_RANGE)
        self.range_error = bool(range_error)
        # bounce_iters (GpuRenderer.adaptive only): rt_stats.bounce_iters summed over the run, a pixel's K once per
        # reduction of that pixel
        self.bounce_iters = int(bounce_iters)
        self._duration = float(duration)
        self._pixels = int(pixels_rendered)
        self._pps = self._pixels / self._duration if self._duration > 0 else 0.0
        self.kernel_ms = kernel_ms
        self.samples = samples
        self.ray_segments = ray_segments

    def duration(self):
        return self._duration

    def pixels_rendered(self):
        return self._pixels

    def pixels_per_second(self):
        return self._pps


class Renderer:
    def render(self, max_bounces, samples_per_pixel, scene, camera):
        raise NotImplementedError


def split_argument(samples_per_item):
    """render_flat's samples_per_item checked: None (rt_render_async), 0 (rt_render_split_async plans) or a
    sample count (forced)."""
    if samples_per_item is None:
        return None
    if isinstance(samples_per_item, bool) or not isinstance(samples_per_item, int):
        raise TypeError(f"samples_per_item must be None or an int, not {samples_per_item!r}")
    if samples_per_item < 0:
        raise ValueError(f"samples_per_item must be >= 0, not {samples_per_item}")
    return samples_per_item


def check_schedule(schedule):
    """A progressive schedule checked before any GPU call: a non-empty, strictly increasing list of positive
    sample counts.  Returns it as a list of ints."""
    counts = list(schedule)
    if not counts:
        raise ValueError("progressive schedule is empty")
    for n in counts:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise ValueError(f"progressive schedule entries must be ints, not {n!r}")
    counts = [int(n) for n in counts]
    if counts[0] < 1:
        raise ValueError(f"progressive schedule must start at 1 sample or more, not {counts[0]}")
    for a, b in zip(counts, counts[1:]):
        if b <= a:
            raise ValueError(f"progressive schedule must be strictly increasing ({a} is followed by {b})")
    return counts


ADAPTIVE_PLANS = ("host", "device")

# Guide buffers (rt_render_guides_async), in the C ABI's argument order, and their channels per pixel.
GUIDE_NAMES = ("albedo", "normal", "depth", "coverage")
GUIDE_CHANNELS = {"albedo": 3, "normal": 3, "depth": 1, "coverage": 1}
Guides = collections.namedtuple("Guides", GUIDE_NAMES)


# Ray-query outputs (rt_query_hits_async), in the C ABI's argument order: name -> (components per ray, dtype; None:
# the rays' precision).
QUERY_NAMES = ("t", "index", "normal", "point", "front")
QUERY_OUTPUTS = {"t": (1, None), "index": (1, np.int32), "normal": (3, None), "point": (3, None), "front": (1, np.uint8)}


def _query_dtype(flags):
    return np.dtype(np.float32 if flags & abi.RT_FLAG_F32 else np.float64)


def _query_shape(name, n):
    return (n, 3) if QUERY_OUTPUTS[name][0] == 3 else (n,)


def check_query(flags, origins, directions, want=QUERY_NAMES):
    """GpuRenderer.query's arguments checked before any GPU call: the live path's hit only (no mode flag), known
    output names, directions (n, 3) and origins (n, 3) or (3,) of finite-or-not numbers (the library judges each
    ray).  Returns (origins, directions, shared, want) with the arrays contiguous in the renderer's precision;
    shared: origins has shape (3,) and is kept in float64 (the library rounds it the way it rounds a camera centre)."""
    if flags & ~(abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2):
        raise ValueError("ray queries are the live path's closest hit: mode 'vectorized2' only (root2 is allowed)")
    want = tuple(want)
    for name in want:
        if name not in QUERY_NAMES:
            raise ValueError(f"unknown query output {name!r} (one of {list(QUERY_NAMES)})")
    if not want:
        raise ValueError("no query output asked for")
    dtype = _query_dtype(flags)
    d = np.asarray(directions)
    o = np.asarray(origins)
    for what, a in (("directions", d), ("origins", o)):
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{what} must be numbers, not dtype {a.dtype}")
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError(f"directions must have shape (n, 3), not {d.shape}")
    shared = o.shape == (3,)
    if not shared and o.shape != d.shape:
        raise ValueError(f"origins must have shape (3,) (one shared origin) or {d.shape} like directions, not {o.shape}")
    if d.shape[0] > 0x7FFFFFFF:
        raise ValueError("more than 0x7FFFFFFF rays in one query")
    o = np.ascontiguousarray(o, dtype=np.float64 if shared else dtype)
    return o, np.ascontiguousarray(d, dtype=dtype), shared, want


def _device_array(obj, what, dtype, shape, device):
    """The device pointer of obj, an object exposing __cuda_array_interface__ (a torch ROCm tensor does), after
    checking dtype, shape, contiguity, writability where it is an output (shape given as an output's) and, where the
    object names one (torch's .device), the device."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError(f"{what} must expose __cuda_array_interface__ (a device array), not {type(obj).__name__}")
    if np.dtype(cai["typestr"]) != np.dtype(dtype):
        raise ValueError(f"{what} must have dtype {np.dtype(dtype).name}, not {np.dtype(cai['typestr']).name}")
    if tuple(cai["shape"]) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, not {tuple(cai['shape'])}")
    strides = cai.get("strides")
    if strides is not None:
        expect, step = [], np.dtype(dtype).itemsize
        for k in reversed(shape):
            expect.insert(0, step)
            step *= max(k, 1)
        if any(s != e for s, e, k in zip(strides, expect, shape) if k > 1):
            raise ValueError(f"{what} must be C-contiguous (strides {tuple(strides)})")
    dev = getattr(obj, "device", None)
    if dev is not None and hasattr(dev, "type"):
        if dev.type != "cuda" or (dev.index is not None and dev.index != device):
            raise ValueError(f"{what} is on {dev}, the renderer's context on device {device}")
    ptr = cai["data"][0]
    if not ptr and int(np.prod(shape)):
        raise ValueError(f"{what} has a NULL data pointer")
    return ptr


def check_query_into(flags, device, origins, directions, outputs):
    """GpuRenderer.query_into's arguments checked before any GPU call.  Returns (n, d_origins | None, origin | None,
    d_directions, {name: pointer})."""
    if flags & ~(abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2):
        raise ValueError("ray queries are the live path's closest hit: mode 'vectorized2' only (root2 is allowed)")
    dtype = _query_dtype(flags)
    cai = getattr(directions, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError(f"directions must expose __cuda_array_interface__ (a device array), not {type(directions).__name__}")
    shape = tuple(cai["shape"])
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"directions must have shape (n, 3), not {shape}")
    n = shape[0]
    if n > 0x7FFFFFFF:
        raise ValueError("more than 0x7FFFFFFF rays in one query")
    d_dir = _device_array(directions, "directions", dtype, (n, 3), device)
    d_org, origin = None, None
    if hasattr(origins, "__cuda_array_interface__"):
        d_org = _device_array(origins, "origins", dtype, (n, 3), device)
    else:
        origin = np.asarray(origins)
        if origin.shape != (3,) or origin.dtype.kind not in "fiu":
            raise ValueError("origins must be a device array of shape (n, 3) or one shared origin of 3 host numbers")
        origin = np.ascontiguousarray(origin, dtype=np.float64)
    ptrs = {}
    for name, obj in outputs.items():
        if obj is None:
            continue
        cw = getattr(obj, "__cuda_array_interface__", None)
        if isinstance(cw, dict) and cw["data"][1]:
            raise ValueError(f"{name} is read-only")
        ptrs[name] = _device_array(obj, name, QUERY_OUTPUTS[name][1] or dtype, _query_shape(name, n), device)
    if not ptrs:
        raise ValueError("no query output given")
    return n, d_org, origin, d_dir, ptrs


def _rays_flags(flags):
    if flags & ~(abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2):
        raise ValueError("caller rays are rendered on the live path: mode 'vectorized2' only (root2 is allowed)")
    return _query_dtype(flags)


def _rays_counts(spp, n, R, pixel_base):
    if isinstance(spp, bool) or not isinstance(spp, (int, np.integer)) or not 1 <= spp <= 1 << 20:
        raise ValueError(f"spp must be an integer in 1..2^20, not {spp!r}")
    if not 1 <= R <= spp:
        raise ValueError(f"rays per pixel must be within 1..spp: directions has {R} rays per pixel, spp is {spp}")
    if n > 0x7FFFFFFF:
        raise ValueError("more than 0x7FFFFFFF pixels in one call")
    if isinstance(pixel_base, bool) or not isinstance(pixel_base, (int, np.integer)) or pixel_base < 0 \
            or pixel_base + n > 1 << 32:
        raise ValueError(f"pixel_base must be an integer with pixel_base + n <= 2^32, not {pixel_base!r}")


def check_render_rays(flags, spp, origins, directions, pixel_base=0):
    """GpuRenderer.render_rays' arguments checked before any GPU call.  directions: (n, R, 3) or (n, 3) (R = 1);
    origins: the same shape, or (3,) for one shared origin.  Returns (origins, directions (n, R, 3), shared), the arrays
    contiguous in the renderer's precision, a shared origin kept in float64."""
    dtype = _rays_flags(flags)
    d = np.asarray(directions)
    o = np.asarray(origins)
    for what, a in (("directions", d), ("origins", o)):
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{what} must be numbers, not dtype {a.dtype}")
    if d.ndim not in (2, 3) or d.shape[-1] != 3:
        raise ValueError(f"directions must have shape (n, R, 3) or (n, 3), not {d.shape}")
    shared = o.shape == (3,)
    if not shared and o.shape != d.shape:
        raise ValueError(f"origins must have shape (3,) (one shared origin) or {d.shape} like directions, not {o.shape}")
    d = d.reshape(d.shape[0], 1, 3) if d.ndim == 2 else d
    _rays_counts(spp, d.shape[0], d.shape[1], pixel_base)
    o = np.ascontiguousarray(o, dtype=np.float64) if shared else np.ascontiguousarray(o, dtype=dtype).reshape(d.shape)
    return o, np.ascontiguousarray(d, dtype=dtype), shared


def check_render_rays_into(flags, device, spp, origins, directions, rgb, linear, pixel_base=0):
    """GpuRenderer.render_rays_into's arguments checked before any GPU call.  Returns (n, R, d_origins | None,
    origin | None, d_directions, d_rgb | None, d_linear | None)."""
    dtype = _rays_flags(flags)
    cai = getattr(directions, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError(f"directions must expose __cuda_array_interface__ (a device array), not {type(directions).__name__}")
    shape = tuple(cai["shape"])
    if len(shape) not in (2, 3) or shape[-1] != 3:
        raise ValueError(f"directions must have shape (n, R, 3) or (n, 3), not {shape}")
    n, R = shape[0], (shape[1] if len(shape) == 3 else 1)
    _rays_counts(spp, n, R, pixel_base)
    d_dir = _device_array(directions, "directions", dtype, shape, device)
    d_org, origin = None, None
    if hasattr(origins, "__cuda_array_interface__"):
        d_org = _device_array(origins, "origins", dtype, shape, device)
    else:
        origin = np.asarray(origins)
        if origin.shape != (3,) or origin.dtype.kind not in "fiu":
            raise ValueError("origins must be a device array shaped like directions or one shared origin of 3 host numbers")
        origin = np.ascontiguousarray(origin, dtype=np.float64)
    ptrs = []
    for name, obj, dt in (("rgb", rgb, np.uint8), ("linear", linear, np.float64)):
        if obj is None:
            ptrs.append(None)
            continue
        cw = getattr(obj, "__cuda_array_interface__", None)
        if isinstance(cw, dict) and cw["data"][1]:
            raise ValueError(f"{name} is read-only")
        ptrs.append(_device_array(obj, name, dt, (n, 3), device))
    if ptrs[0] is None and ptrs[1] is None:
        raise ValueError("no output given (rgb or linear)")
    return n, R, d_org, origin, d_dir, ptrs[0], ptrs[1]


def check_adaptive(spp_min, spp_max, tolerance, plan="host"):
    """GpuRenderer.adaptive's arguments checked before any GPU call: 1 <= spp_min <= spp_max, a tolerance that is
    a number (not NaN), a plan that is "host" or "device".  Returns (spp_min, spp_max, tolerance) as
    (int, int, float)."""
    if plan not in ADAPTIVE_PLANS:
        raise ValueError(f"unknown plan {plan!r} (one of {list(ADAPTIVE_PLANS)})")
    for name, n in (("spp_min", spp_min), ("spp_max", spp_max)):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise ValueError(f"{name} must be an int, not {n!r}")
    if spp_min < 1:
        raise ValueError(f"spp_min must be 1 or more, not {spp_min}")
    if spp_min > spp_max:
        raise ValueError(f"spp_min ({spp_min}) is above spp_max ({spp_max})")
    tolerance = float(tolerance)
    if tolerance != tolerance:
        raise ValueError("tolerance is NaN")
    return int(spp_min), int(spp_max), tolerance


class ProgressiveSession:
    """One progressive session on a GpuRenderer's context (rt_progressive_*, include/rt_mi355x.h): the
    samples traced so far stay in a record buffer, extend() adds more and takes an image at any count.  The
    image after n samples is bit for bit render_flat's at spp = n.  extend_map() gives every pixel a count of
    its own (pixel p's value is render_flat's at spp = counts[p]), snapshot() reduces at any earlier counts and
    error() is the half-buffer estimate adaptive sampling steers by.  Pixels are indexed in the range's compact
    order, the order of the outputs.  A context manager; close() frees the buffer."""

    def __init__(self, renderer, max_bounces, spp_capacity, flat, cam, tile_range=None, max_bytes=0):
        self.renderer, self.lib = renderer, renderer.lib
        self.capacity = int(spp_capacity)
        self._open = False
        if renderer._scene_flat is not flat:
            renderer.set_scene(flat)
        tr = tile_range if tile_range is not None else abi.RtTileRange(0, 1, cam.image_height, 0, cam.image_width)
        self.npx = tr.row_count * tr.col_count
        self._counts = np.zeros(self.npx, dtype=np.uint32)
        self._stale = False   # refine() moved counts on the device since _counts was read
        abi.check(self.lib, self.lib.rt_progressive_begin(renderer.ctx, ctypes.byref(cam), max_bounces, spp_capacity,
                                                          renderer.seed, renderer.flags, ctypes.byref(tr), max_bytes))
        self._open = True
        renderer._session = self

    @property
    def counts(self):
        """Samples traced so far per pixel: np.uint32[n] (a copy)."""
        if self._stale and self._open:
            self._refresh()
        return self._counts.copy()

    @property
    def done(self):
        """Samples every pixel holds: the minimum over the pixels (a uniform session: its sample count)."""
        if self._stale and self._open:
            self._refresh()
        return int(self._counts.min())

    def _refresh(self):
        abi.check(self.lib, self.lib.rt_progressive_counts(self.renderer.ctx,
                                                           self._counts.ctypes.data_as(ctypes.POINTER(abi.u32))))
        self._stale = False

    def _map_argument(self, counts, what):
        a = np.ascontiguousarray(counts)
        if a.shape != (self.npx,) or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
            raise ValueError(f"{what} must be {self.npx} unsigned sample counts, one per pixel of the session's range")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def _run(self, call, want_linear, image, stream):
        """call(d_rgb8, d_linear) on fresh device buffers, then collect and read back: (rgb [n,3] u8, linear
        [n,3] f64 | None, RtStats, rc); image=False: no buffers, returns the RtStats."""
        if not self._open:
            raise RuntimeError("the progressive session is closed")
        lib, ctx = self.lib, self.renderer.ctx
        d_rgb, d_lin = ctypes.c_void_p(), ctypes.c_void_p()
        try:
            if image:
                abi.check(lib, lib.rt_device_alloc(ctx, self.npx * 3, ctypes.byref(d_rgb)))
                if want_linear:
                    abi.check(lib, lib.rt_device_alloc(ctx, self.npx * 3 * 8, ctypes.byref(d_lin)))
            abi.check(lib, call(d_rgb if image else None, d_lin if image and want_linear else None))
            self._refresh()
            st = abi.RtStats()
            rc = abi.check(lib, lib.rt_context_collect(ctx, stream, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
            if not image:
                return st
            rgb = np.empty((self.npx, 3), dtype=np.uint8)
            abi.check(lib, lib.rt_memcpy_d2h(ctx, rgb.ctypes.data, d_rgb, self.npx * 3))
            lin = None
            if want_linear:
                lin = np.empty((self.npx, 3), dtype=np.float64)
                abi.check(lib, lib.rt_memcpy_d2h(ctx, lin.ctypes.data, d_lin, self.npx * 3 * 8))
        finally:
            if d_rgb:
                lib.rt_device_free(ctx, d_rgb)
            if d_lin:
                lib.rt_device_free(ctx, d_lin)
        return rgb, lin, st, rc

    def extend(self, spp_total, want_linear=False, image=True, stream=None):
        """Trace samples [done, spp_total) and reduce [0, spp_total): (rgb [n,3] u8, linear [n,3] f64 | None,
        RtStats, rc) like render_flat; rc is RT_OK or RT_ERR_RANGE.  image=False: trace only, returns the RtStats."""
        ctx = self.renderer.ctx
        return self._run(lambda rgb, lin: self.lib.rt_progressive_extend_async(ctx, spp_total, rgb, lin, stream),
                         want_linear, image, stream)

    def extend_map(self, targets, want_linear=False, image=True, stream=None):
        """rt_progressive_extend_map_async: trace samples [counts[p], targets[p]) of every pixel p and reduce pixel
        p at targets[p].  Returns what extend() returns."""
        t = self._map_argument(targets, "targets")
        ctx, tp = self.renderer.ctx, t.ctypes.data_as(ctypes.POINTER(abi.u32))
        return self._run(lambda rgb, lin: self.lib.rt_progressive_extend_map_async(ctx, tp, rgb, lin, stream),
                         want_linear, image, stream)

    def snapshot(self, counts=None, want_linear=False, stream=None):
        """rt_progressive_snapshot_map_async: the image with pixel p at counts[p] <= its samples so far (None: at
        every pixel's own count), nothing traced.  (rgb, linear | None, RtStats, rc)."""
        c = None if counts is None else self._map_argument(counts, "counts")
        ctx, cp = self.renderer.ctx, None if c is None else c.ctypes.data_as(ctypes.POINTER(abi.u32))
        return self._run(lambda rgb, lin: self.lib.rt_progressive_snapshot_map_async(ctx, cp, rgb, lin, stream),
                         want_linear, True, stream)

    def error(self, stream=None, stats=False):
        """rt_progressive_error_async: np.float64[n], per pixel the largest channel difference between its linear
        value at counts[p] and at counts[p] // 2 samples; inf below 2 samples.  stats=True: (error, RtStats)."""
        if not self._open:
            raise RuntimeError("the progressive session is closed")
        lib, ctx = self.lib, self.renderer.ctx
        d_err = ctypes.c_void_p()
        abi.check(lib, lib.rt_device_alloc(ctx, self.npx * 8, ctypes.byref(d_err)))
        try:
            abi.check(lib, lib.rt_progressive_error_async(ctx, d_err, stream))
            st = abi.RtStats()
            abi.check(lib, lib.rt_context_collect(ctx, stream, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
            err = np.empty(self.npx, dtype=np.float64)
            abi.check(lib, lib.rt_memcpy_d2h(ctx, err.ctypes.data, d_err, self.npx * 8))
        finally:
            lib.rt_device_free(ctx, d_err)
        return (err, st) if stats else err

    def refine(self, tolerance, spp_max, stream=None):
        """rt_progressive_refine: one step of the doubling policy, selected and planned on the device.  Returns
        (n_active, n_samples): the pixels whose estimate was above `tolerance` and that went to
        min(2 * count, spp_max), and the samples enqueued for them; n_active == 0: converged, nothing traced.  The
        call waits for the selection (one small readback), not for the tracing: collect() follows."""
        if not self._open:
            raise RuntimeError("the progressive session is closed")
        na, ns = abi.u64(), abi.u64()
        abi.check(self.lib, self.lib.rt_progressive_refine(self.renderer.ctx, float(tolerance), int(spp_max), stream,
                                                           ctypes.byref(na), ctypes.byref(ns)))
        self._stale = True
        return na.value, ns.value

    def refine_items(self):
        """rt_progressive_refine_items: (samples_per_item, items np.uint32[n, 4] of pixel, first, end, 0) of the
        item table the last refine() built on the device; (0, empty) when it selected nothing."""
        if not self._open:
            raise RuntimeError("the progressive session is closed")
        lib, ctx, U32P = self.lib, self.renderer.ctx, ctypes.POINTER(abi.u32)
        s, n = abi.u32(), abi.u64()
        abi.check(lib, lib.rt_progressive_refine_items(ctx, ctypes.byref(s), ctypes.byref(n), None, 0))
        items = np.zeros((n.value, 4), dtype=np.uint32)
        if n.value:
            abi.check(lib, lib.rt_progressive_refine_items(ctx, ctypes.byref(s), ctypes.byref(n),
                                                           items.ctypes.data_as(U32P), n.value))
        return s.value, items

    def collect(self, stream=None):
        """rt_context_collect: wait for the work enqueued on `stream` and return its RtStats (a channel above 2.0 in
        one of its reductions is not an error here)."""
        st = abi.RtStats()
        abi.check(self.lib, self.lib.rt_context_collect(self.renderer.ctx, stream, ctypes.byref(st)),
                  allow=(abi.RT_ERR_RANGE,))
        return st

    def close(self):
        if self._open:
            self._open = False
            if self.renderer._session is self:
                self.renderer._session = None
            if self.renderer.ctx:   # rt_context_destroy has ended it otherwise
                abi.check(self.lib, self.lib.rt_progressive_end(self.renderer.ctx))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class GpuRenderer(Renderer):
    """Drop-in for TileRenderer: renders the whole image on one MI355X via rt_render_async.

    seed: 64-bit key of the counter-based RNG (the reference's thread_rng is unseedable);
    precision: "f64" (reference arithmetic) or "f32"; root2: quirk Q1 off;
    mode: which reference renderer to reproduce — "vectorized2" (the live render_vectorized2,
    default), "vectorized" (render_vectorized), "vectorized3" (render_vectorized3) or "scalar" (render);
    see include/rt_mi355x.h.
    sample_parallel: render() deals each pixel's samples to several waves where the frame has fewer pixels
    than the chip has waves (rt_render_split_async's auto plan; the live path only, same image).
    """

    MODES = {"vectorized2": 0, "vectorized": abi.RT_FLAG_MODE_VECTORIZED, "vectorized3": abi.RT_FLAG_MODE_VECTORIZED3,
             "scalar": abi.RT_FLAG_MODE_SCALAR}

    def __init__(self, device=0, seed=0x5EED0001, precision="f64", root2=False, mode="vectorized2", lib=None,
                 sample_parallel=False):
        if mode not in self.MODES:
            raise ValueError(f"unknown mode {mode!r} (one of {sorted(self.MODES)})")
        if precision not in ("f64", "f32"):
            raise ValueError(f"unknown precision {precision!r}")
        self.lib = lib or abi.load_library()
        self.device = device
        self.sample_parallel = bool(sample_parallel)
        self.seed = seed
        self.flags = ((abi.RT_FLAG_F32 if precision == "f32" else 0) | (abi.RT_FLAG_ROOT2 if root2 else 0)
                      | self.MODES[mode])
        self.ctx = ctypes.c_void_p()
        abi.check(self.lib, self.lib.rt_context_create(device, ctypes.byref(self.ctx)))
        self._scene_flat = None   # the FlatScene last uploaded (held, so its identity cannot be reused)
        self._session = None      # the open ProgressiveSession, if any (one per context)

    def close(self):
        if self.ctx:
            if self._session is not None:   # rt_context_destroy ends it
                self._session._open = False
                self._session = None
            self.lib.rt_context_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, flat):
        # rt_context_set_scene frees the previous scene before uploading this one: if the upload fails
        # the context holds no usable scene, so the cache must not point at the previous one either.
        self._scene_flat = None
        abi.check(self.lib, self.lib.rt_context_set_scene(self.ctx, ctypes.byref(flat.abi)))
        # A strong reference, compared with `is`: an id() key could match a new FlatScene that CPython
        # allocated at a freed one's address, and the render would silently use the old spheres.
        self._scene_flat = flat

    def render_flat(self, max_bounces, spp, flat, cam, tile_range=None, want_linear=False, samples_per_item=None):
        """Render with a FlatScene / RtCamera; returns (rgb [n,3] u8, linear [n,3] f64 | None, RtStats, rc).
        samples_per_item: None = rt_render_async; 0 = rt_render_split_async with its own plan; n > 0 = that many
        samples per work item (the sample-parallel path, include/rt_mi355x.h)."""
        lib = self.lib
        split = split_argument(samples_per_item)
        if self._scene_flat is not flat:
            self.set_scene(flat)
        if tile_range is None:
            tr = abi.RtTileRange(0, 1, cam.image_height, 0, cam.image_width)
        else:
            tr = tile_range
        npx = tr.row_count * tr.col_count
        d_rgb, d_lin = ctypes.c_void_p(), ctypes.c_void_p()
        abi.check(lib, lib.rt_device_alloc(self.ctx, npx * 3, ctypes.byref(d_rgb)))
        try:
            if want_linear:
                abi.check(lib, lib.rt_device_alloc(self.ctx, npx * 3 * 8, ctypes.byref(d_lin)))
            if split is None:
                abi.check(lib, lib.rt_render_async(self.ctx, ctypes.byref(cam), max_bounces, spp, self.seed, self.flags,
                                                   ctypes.byref(tr), d_rgb, d_lin if want_linear else None, None))
            else:
                abi.check(lib, lib.rt_render_split_async(self.ctx, ctypes.byref(cam), max_bounces, spp, self.seed,
                                                         self.flags, ctypes.byref(tr), d_rgb,
                                                         d_lin if want_linear else None, None, split))
            st = abi.RtStats()
            rc = abi.check(lib, lib.rt_context_collect(self.ctx, None, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
            rgb = np.empty((npx, 3), dtype=np.uint8)
            abi.check(lib, lib.rt_memcpy_d2h(self.ctx, rgb.ctypes.data, d_rgb, npx * 3))
            lin = None
            if want_linear:
                lin = np.empty((npx, 3), dtype=np.float64)
                abi.check(lib, lib.rt_memcpy_d2h(self.ctx, lin.ctypes.data, d_lin, npx * 3 * 8))
        finally:
            lib.rt_device_free(self.ctx, d_rgb)
            if want_linear and d_lin:
                lib.rt_device_free(self.ctx, d_lin)
        return rgb, lin, st, rc

    def render(self, max_bounces, samples_per_pixel, scene, camera):
        t0 = time.perf_counter()
        flat = scene.flatten() if hasattr(scene, "flatten") else scene
        cam = camera.abi if hasattr(camera, "abi") else camera
        rgb, _, st, rc = self.render_flat(max_bounces, samples_per_pixel, flat, cam,
                                          samples_per_item=0 if self.sample_parallel else None)
        dt = time.perf_counter() - t0
        if rc == abi.RT_ERR_RANGE:
            raise abi.RtError(rc, "a pixel channel exceeded 2.0 (reference: Color::to_u8_array panics)")
        img = rgb.reshape(cam.image_height, cam.image_width, 3)
        return img, RenderStat(dt, cam.image_width * cam.image_height, st.kernel_ms, st.samples, st.ray_segments)

    def _check_guides(self, want=GUIDE_NAMES):
        """The guide calls' arguments checked before any GPU call: the live path only, known output names."""
        if self.flags & ~abi.RT_FLAG_F32:
            raise ValueError("guide buffers are the live path's first hits: mode 'vectorized2' without root2 only")
        want = tuple(want)
        for name in want:
            if name not in GUIDE_NAMES:
                raise ValueError(f"unknown guide buffer {name!r} (one of {list(GUIDE_NAMES)})")
        if not want:
            raise ValueError("no guide buffer asked for")
        return want

    def guides_flat(self, spp, flat, cam, tile_range=None, want=GUIDE_NAMES):
        """rt_render_guides_async with a FlatScene / RtCamera: per pixel the mean first-hit albedo, normal, depth and
        coverage over the primary rays of render_flat's image at `spp` (the renderer's seed and precision; the
        definition is in include/rt_mi355x.h).  Returns ({name: float32 array, flat over the range}, RtStats, rc):
        albedo and normal [n, 3], depth and coverage [n].  want: the buffers to compute the outputs of (a value
        does not depend on which others are asked for)."""
        want = self._check_guides(want)
        lib = self.lib
        if self._scene_flat is not flat:
            self.set_scene(flat)
        tr = tile_range if tile_range is not None else abi.RtTileRange(0, 1, cam.image_height, 0, cam.image_width)
        npx = tr.row_count * tr.col_count
        dev = {name: ctypes.c_void_p() for name in want}
        out = {}
        try:
            for name in want:
                abi.check(lib, lib.rt_device_alloc(self.ctx, npx * GUIDE_CHANNELS[name] * 4, ctypes.byref(dev[name])))
            abi.check(lib, lib.rt_render_guides_async(self.ctx, ctypes.byref(cam), spp, self.seed, self.flags,
                                                      ctypes.byref(tr), *[dev.get(name) for name in GUIDE_NAMES], None))
            st = abi.RtStats()
            rc = abi.check(lib, lib.rt_context_collect(self.ctx, None, ctypes.byref(st)))
            for name in want:
                ch = GUIDE_CHANNELS[name]
                a = np.empty((npx, ch) if ch > 1 else (npx,), dtype=np.float32)
                abi.check(lib, lib.rt_memcpy_d2h(self.ctx, a.ctypes.data, dev[name], npx * ch * 4))
                out[name] = a
        finally:
            for d in dev.values():
                if d:
                    lib.rt_device_free(self.ctx, d)
        return out, st, rc

    def guides(self, spp, scene, camera):
        """The guide buffers of render()'s image at `spp` samples: (Guides(albedo (H, W, 3), normal (H, W, 3),
        depth (H, W), coverage (H, W)) of float32, RenderStat).  The means are over all samples of a pixel, so
        they are premultiplied by coverage."""
        self._check_guides()   # before any GPU call
        t0 = time.perf_counter()
        flat = scene.flatten() if hasattr(scene, "flatten") else scene
        cam = camera.abi if hasattr(camera, "abi") else camera
        out, st, _ = self.guides_flat(spp, flat, cam)
        dt = time.perf_counter() - t0
        h, w = cam.image_height, cam.image_width
        g = Guides(out["albedo"].reshape(h, w, 3), out["normal"].reshape(h, w, 3), out["depth"].reshape(h, w),
                   out["coverage"].reshape(h, w))
        return g, RenderStat(dt, w * h, st.kernel_ms, st.samples, st.ray_segments)

    def _query_flags(self, root2):
        return self.flags | (abi.RT_FLAG_ROOT2 if root2 else 0)

    def query(self, origins, directions, scene, root2=False, want=QUERY_NAMES):
        """rt_query_hits_async with numpy arrays: the closest hit of each ray (include/rt_mi355x.h has the
        definition).  directions: (n, 3), not normalised; origins: (n, 3), or (3,) for one shared origin (the camera
        sweep over that origin's tables: the same values, and no origins to upload or read).  The arrays are
        converted to the renderer's precision.  root2: quirk Q1 off, what picking wants (a ray that starts inside a
        sphere then hits it from the inside); a renderer made with root2=True always has it.
        Returns {name: array} for the names in `want`: t (n,) and normal, point (n, 3) in the renderer's precision,
        index (n,) int32 (abi.RT_QUERY_MISS = -1: no hit; abi.RT_QUERY_INVALID = -2: a ray outside the precondition,
        not traced, its t NaN), front (n,) uint8.  The call's RtStats are kept in self.query_stats."""
        flags = self._query_flags(root2)
        o, d, shared, want = check_query(flags, origins, directions, want)   # before any GPU call
        n = d.shape[0]
        dtype = d.dtype
        out = {name: np.empty(_query_shape(name, n), dtype=QUERY_OUTPUTS[name][1] or dtype) for name in want}
        flat = scene.flatten() if hasattr(scene, "flatten") else scene
        lib = self.lib
        if self._scene_flat is not flat:
            self.set_scene(flat)
        if n == 0:
            self.query_stats = abi.RtStats()
            return out
        dev = {name: ctypes.c_void_p() for name in want}
        d_dir, d_org = ctypes.c_void_p(), ctypes.c_void_p()
        try:
            abi.check(lib, lib.rt_device_alloc(self.ctx, d.nbytes, ctypes.byref(d_dir)))
            abi.check(lib, lib.rt_memcpy_h2d(self.ctx, d_dir, d.ctypes.data, d.nbytes))
            if not shared:
                abi.check(lib, lib.rt_device_alloc(self.ctx, o.nbytes, ctypes.byref(d_org)))
                abi.check(lib, lib.rt_memcpy_h2d(self.ctx, d_org, o.ctypes.data, o.nbytes))
            for name in want:
                abi.check(lib, lib.rt_device_alloc(self.ctx, out[name].nbytes, ctypes.byref(dev[name])))
            origin = o.ctypes.data_as(ctypes.POINTER(abi.f64)) if shared else None
            abi.check(lib, lib.rt_query_hits_async(self.ctx, n, None if shared else d_org, origin, d_dir, flags,
                                                   *[dev.get(name) for name in QUERY_NAMES], None))
            st = abi.RtStats()
            abi.check(lib, lib.rt_context_collect(self.ctx, None, ctypes.byref(st)))
            self.query_stats = st
            for name in want:
                abi.check(lib, lib.rt_memcpy_d2h(self.ctx, out[name].ctypes.data, dev[name], out[name].nbytes))
        finally:
            for p in [d_dir, d_org] + list(dev.values()):
                if p:
                    lib.rt_device_free(self.ctx, p)
        return out

    def query_into(self, origins, directions, *, t=None, index=None, normal=None, point=None, front=None, stream=None,
                   root2=False):
        """rt_query_hits_async on device arrays in place, without a copy: directions (n, 3) and every output given
        are objects exposing __cuda_array_interface__ (torch ROCm tensors do) in the renderer's precision, C-contiguous,
        on the renderer's device; index is int32 and front uint8.  origins: such an array of shape (n, 3), or 3 host
        numbers for one shared origin.  The scene is the one last set (set_scene).  stream: an integer stream handle
        such as torch.cuda.current_stream().cuda_stream (None: the null stream); the call is asynchronous on it, so
        the caller orders its own reads after it on that stream.  Returns the number of rays."""
        flags = self._query_flags(root2)
        n, d_org, origin, d_dir, ptrs = check_query_into(
            flags, self.device, origins, directions, dict(t=t, index=index, normal=normal, point=point, front=front))
        if stream is not None and (isinstance(stream, bool) or not isinstance(stream, int)):
            raise TypeError(f"stream must be an integer stream handle or None, not {stream!r}")
        if self._scene_flat is None:
            raise RuntimeError("query_into needs a scene: call set_scene first")
        op = origin.ctypes.data_as(ctypes.POINTER(abi.f64)) if origin is not None else None
        abi.check(self.lib, self.lib.rt_query_hits_async(self.ctx, n, d_org, op, d_dir, flags,
                                                         *[ptrs.get(name) for name in QUERY_NAMES], stream))
        return n

    def render_rays(self, max_bounces, spp, origins, directions, scene, seed=None, pixel_base=0, root2=False,
                    want_linear=False):
        """rt_render_rays_async with numpy arrays: full paths for caller-supplied primary rays (include/rt_mi355x.h
        has the definition; rt_mi355x.projections makes the rays of an orthographic, panorama or fisheye camera).
        directions: (n, R, 3), or (n, 3) for one ray per pixel, not normalised; sample s of pixel p starts as ray
        s % R of that pixel.  origins: the same shape, or (3,) for one shared origin.  seed: the RNG key (None: the
        renderer's); pixel_base: the RNG's pixel of pixel 0 (shards of one frame pass their first pixel).  A pixel
        with an invalid ray (non-finite, or |d|^2 outside [1e-6, 1e6]) comes back black, its linear value NaN.
        Returns (rgb [n, 3] u8, linear [n, 3] f64 | None, RtStats, rc)."""
        flags = self._query_flags(root2)
        o, d, shared = check_render_rays(flags, spp, origins, directions, pixel_base)   # before any GPU call
        n, R = d.shape[0], d.shape[1]
        flat = scene.flatten() if hasattr(scene, "flatten") else scene
        lib = self.lib
        if self._scene_flat is not flat:
            self.set_scene(flat)
        rgb = np.empty((n, 3), dtype=np.uint8)
        lin = np.empty((n, 3), dtype=np.float64) if want_linear else None
        if n == 0:
            return rgb, lin, abi.RtStats(), abi.RT_OK
        d_dir, d_org, d_rgb, d_lin = (ctypes.c_void_p() for _ in range(4))
        try:
            abi.check(lib, lib.rt_device_alloc(self.ctx, d.nbytes, ctypes.byref(d_dir)))
            abi.check(lib, lib.rt_memcpy_h2d(self.ctx, d_dir, d.ctypes.data, d.nbytes))
            if not shared:
                abi.check(lib, lib.rt_device_alloc(self.ctx, o.nbytes, ctypes.byref(d_org)))
                abi.check(lib, lib.rt_memcpy_h2d(self.ctx, d_org, o.ctypes.data, o.nbytes))
            abi.check(lib, lib.rt_device_alloc(self.ctx, n * 3, ctypes.byref(d_rgb)))
            if want_linear:
                abi.check(lib, lib.rt_device_alloc(self.ctx, n * 3 * 8, ctypes.byref(d_lin)))
            origin = o.ctypes.data_as(ctypes.POINTER(abi.f64)) if shared else None
            abi.check(lib, lib.rt_render_rays_async(self.ctx, n, spp, R, None if shared else d_org, origin, d_dir,
                                                    max_bounces, self.seed if seed is None else seed, pixel_base, flags,
                                                    d_rgb, d_lin if want_linear else None, None))
            st = abi.RtStats()
            rc = abi.check(lib, lib.rt_context_collect(self.ctx, None, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
            abi.check(lib, lib.rt_memcpy_d2h(self.ctx, rgb.ctypes.data, d_rgb, n * 3))
            if want_linear:
                abi.check(lib, lib.rt_memcpy_d2h(self.ctx, lin.ctypes.data, d_lin, n * 3 * 8))
        finally:
            for p in (d_dir, d_org, d_rgb, d_lin):
                if p:
                    lib.rt_device_free(self.ctx, p)
        return rgb, lin, st, rc

    def render_rays_into(self, max_bounces, spp, origins, directions, *, rgb=None, linear=None, seed=None, pixel_base=0,
                         root2=False, stream=None):
        """rt_render_rays_async on device arrays in place, without a copy: directions (n, R, 3) or (n, 3) and the
        outputs given (rgb (n, 3) uint8, linear (n, 3) float64) are objects exposing __cuda_array_interface__ (torch
        ROCm tensors do), C-contiguous, on the renderer's device, the rays in the renderer's precision.  origins: such
        an array shaped like directions, or 3 host numbers for one shared origin.  The scene is the one last set
        (set_scene).  stream: an integer stream handle (None: the null stream); the call is asynchronous on it, and
        collect-time errors (RT_ERR_RANGE) are the caller's to collect.  Returns the number of pixels."""
        flags = self._query_flags(root2)
        n, R, d_org, origin, d_dir, d_rgb, d_lin = check_render_rays_into(
            flags, self.device, spp, origins, directions, rgb, linear, pixel_base)
        if stream is not None and (isinstance(stream, bool) or not isinstance(stream, int)):
            raise TypeError(f"stream must be an integer stream handle or None, not {stream!r}")
        if self._scene_flat is None:
            raise RuntimeError("render_rays_into needs a scene: call set_scene first")
        op = origin.ctypes.data_as(ctypes.POINTER(abi.f64)) if origin is not None else None
        abi.check(self.lib, self.lib.rt_render_rays_async(self.ctx, n, spp, R, d_org, op, d_dir, max_bounces,
                                                          self.seed if seed is None else seed, pixel_base, flags,
                                                          d_rgb, d_lin, stream))
        return n

    def begin_progressive(self, max_bounces, spp_capacity, scene, camera, tile_range=None, max_bytes=0):
        """Open a ProgressiveSession (rt_progressive_begin) for up to spp_capacity samples per pixel.  The live
        path only: mode "vectorized2" without root2.  max_bytes: the most the record buffer may take
        (0 = the library's 24 GB budget; see rt_progressive_bytes for the cost)."""
        flat = scene.flatten() if hasattr(scene, "flatten") else scene
        cam = camera.abi if hasattr(camera, "abi") else camera
        return ProgressiveSession(self, max_bounces, spp_capacity, flat, cam, tile_range, max_bytes)

    def progressive(self, max_bounces, schedule, scene, camera):
        """Render at each sample count of `schedule` (strictly increasing), tracing only the new samples of
        each step: yields (spp, image HxWx3 uint8, RenderStat) per step, every image equal to render()'s at
        that spp.  A step whose image has a channel above 2.0 (RT_ERR_RANGE; at 1 spp the reference's own
        arithmetic gets there) is yielded with stat.range_error set instead of raising, so that a preview
        never aborts the run.  The stat's samples and ray_segments are those of the step."""
        counts = check_schedule(schedule)   # before any GPU call
        return self._progressive(max_bounces, counts, scene, camera)

    def _progressive(self, max_bounces, counts, scene, camera):
        cam = camera.abi if hasattr(camera, "abi") else camera
        with self.begin_progressive(max_bounces, counts[-1], scene, cam) as session:
            for n in counts:
                t0 = time.perf_counter()
                rgb, _, st, rc = session.extend(n)
                dt = time.perf_counter() - t0
                img = rgb.reshape(cam.image_height, cam.image_width, 3)
                yield n, img, RenderStat(dt, cam.image_width * cam.image_height, st.kernel_ms, st.samples,
                                         st.ray_segments, range_error=rc == abi.RT_ERR_RANGE)

    def adaptive(self, max_bounces, spp_min, spp_max, tolerance, scene, camera, plan="host"):
        """Adaptive sampling: every pixel gets spp_min samples, then the pixels whose error estimate
        (ProgressiveSession.error) is above `tolerance` double their count, up to spp_max, until none is left.
        Returns (image HxWx3 uint8, counts HxW uint32, RenderStat); pixel p of the image equals render()'s at
        spp = counts[p], and stat.samples is the total traced (counts.sum()).  The live path only.
        plan: "host" estimates the whole frame, selects in numpy and sends a map per step; "device" keeps the
        estimate, the selection and the item table on the GPU (ProgressiveSession.refine) and reads the counts
        back once, at the end.  Same counts, same image."""
        spp_min, spp_max, tolerance = check_adaptive(spp_min, spp_max, tolerance, plan)   # before any GPU call
        t0 = time.perf_counter()
        cam = camera.abi if hasattr(camera, "abi") else camera
        ms, samples, segs, iters = 0.0, 0, 0, 0

        def add(st):
            nonlocal ms, samples, segs, iters
            ms, samples, segs = ms + st.kernel_ms, samples + st.samples, segs + st.ray_segments
            iters += st.bounce_iters

        with self.begin_progressive(max_bounces, spp_max, scene, cam) as session:
            add(session.extend(spp_min, image=False))
            if plan == "device":
                while session.refine(tolerance, spp_max)[0]:   # each step waits for its selection only
                    pass
                add(session.collect())   # a half-count reduction above 2.0 is not the image's
            while plan == "host":
                err, st = session.error(stats=True)
                add(st)
                counts = session.counts
                active = (err > tolerance) & (counts < spp_max)
                if not active.any():
                    break
                counts[active] = np.minimum(2 * counts[active].astype(np.uint64), spp_max).astype(np.uint32)
                add(session.extend_map(counts, image=False))
            rgb, _, st, rc = session.snapshot()
            add(st)
            counts = session.counts
        dt = time.perf_counter() - t0
        if rc == abi.RT_ERR_RANGE:
            raise abi.RtError(rc, "a pixel channel exceeded 2.0 (reference: Color::to_u8_array panics)")
        h, w = cam.image_height, cam.image_width
        return rgb.reshape(h, w, 3), counts.reshape(h, w), RenderStat(dt, w * h, ms, samples, segs, bounce_iters=iters)
