"""Renderer trait mirror (src/renderer.rs:11-40) backed by the MI355X C ABI.

    trait Renderer { fn render(&self, max_bounces, samples_per_pixel, &Arc<Scene>, &Arc<Camera>)
                     -> (RgbImage, RenderStat) }                       renderer.rs:38-40
    TileRenderer::new(num_threads: Option<NonZeroUsize>, block_size)   renderer.rs:232-241

`GpuRenderer.render` has the same argument meaning and returns (image HxWx3 uint8 numpy array,
RenderStat).  Where the reference panics (Color::to_u8_array's `<= 2.0` assert,
color.rs:55-57; unknown material, materials.rs:31; spp == 0 -> 0/0) this raises RtError.
There is no CPU fallback: the HIP library must be built and a GPU present.

Every method checks its arguments (checks.py) before it touches the library, the context or the scene.  A method
that reads results back does so in one abi.DeviceScope: allocate, launch, abi.collect, download.
"""
import ctypes
import time

import numpy as np

from . import abi
from .checks import (ADAPTIVE_PLANS, GUIDE_CHANNELS, GUIDE_NAMES, QUERY_NAMES, QUERY_OUTPUTS, Guides,  # noqa: F401
                     _device_array, _query_shape, check_adaptive, check_guides, check_query, check_query_into,
                     check_render_rays, check_render_rays_into, check_schedule, check_stream, split_argument)
from .list_checks import check_compact_list_into, check_path_step_list_into
from .occlusion_checks import check_occluded, check_occluded_into, check_scene_set  # noqa: F401
from .step_checks import (STEP_NAMES, STEP_OUTPUTS, _step_shape, check_path_step, check_path_step_into,  # noqa: F401
                          check_scatter, check_scatter_into, check_seed, check_step_names)
from .step_checks import check_scene_set as check_step_scene


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


def _flat(scene):
    return scene.flatten() if hasattr(scene, "flatten") else scene


def _abi_camera(camera):
    return camera.abi if hasattr(camera, "abi") else camera


def _range(cam, tile_range=None):
    """tile_range, or the whole image of cam."""
    return tile_range if tile_range is not None else abi.RtTileRange(0, 1, cam.image_height, 0, cam.image_width)


def _pointer(a, ctype):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctype))


def _render_stat(t0, cam, st, **kw):
    """The RenderStat of a whole image of cam begun at t0, its work counters from an RtStats."""
    return RenderStat(time.perf_counter() - t0, cam.image_width * cam.image_height, st.kernel_ms, st.samples,
                      st.ray_segments, **kw)


def _raise_range(rc):
    if rc == abi.RT_ERR_RANGE:
        raise abi.RtError(rc, "a pixel channel exceeded 2.0 (reference: Color::to_u8_array panics)")


def _read_image(dev, n, want_linear, launch, stream=None, before_collect=None):
    """launch(d_rgb8, d_linear) on fresh buffers of the DeviceScope dev for n pixels, then collect on `stream` and
    read back: (rgb [n,3] u8, linear [n,3] f64 | None, RtStats, rc); rc is RT_OK or RT_ERR_RANGE."""
    d_rgb = dev.alloc(n * 3)
    d_lin = dev.alloc(n * 3 * 8) if want_linear else None
    abi.check(dev.lib, launch(d_rgb, d_lin))
    if before_collect is not None:
        before_collect()
    st, rc = abi.collect(dev.lib, dev.ctx, stream, allow_range=True)
    rgb = dev.download(d_rgb, np.empty((n, 3), dtype=np.uint8))
    lin = dev.download(d_lin, np.empty((n, 3), dtype=np.float64)) if want_linear else None
    return rgb, lin, st, rc


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
        renderer._use_scene(flat)
        tr = _range(cam, tile_range)
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
        abi.check(self.lib, self.lib.rt_progressive_counts(self.renderer.ctx, _pointer(self._counts, abi.u32)))
        self._stale = False

    def _require_open(self):
        if not self._open:
            raise RuntimeError("the progressive session is closed")

    def _map_argument(self, counts, what):
        a = np.ascontiguousarray(counts)
        if a.shape != (self.npx,) or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
            raise ValueError(f"{what} must be {self.npx} unsigned sample counts, one per pixel of the session's range")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def _run(self, launch, want_linear, image, stream):
        """launch(d_rgb8, d_linear), the counts read again, then collect and read back: what _read_image returns;
        image=False: no buffers, returns the RtStats."""
        self._require_open()
        lib, ctx = self.lib, self.renderer.ctx
        if not image:
            abi.check(lib, launch(None, None))
            self._refresh()
            return abi.collect(lib, ctx, stream, allow_range=True)[0]
        with abi.DeviceScope(lib, ctx) as dev:
            return _read_image(dev, self.npx, want_linear, launch, stream, before_collect=self._refresh)

    def extend(self, spp_total, want_linear=False, image=True, stream=None):
        """Trace samples [done, spp_total) and reduce [0, spp_total): (rgb [n,3] u8, linear [n,3] f64 | None,
        RtStats, rc) like render_flat; rc is RT_OK or RT_ERR_RANGE.  image=False: trace only, returns the RtStats."""
        ctx = self.renderer.ctx
        return self._run(lambda rgb, lin: self.lib.rt_progressive_extend_async(ctx, spp_total, rgb, lin, stream),
                         want_linear, image, stream)

    def extend_map(self, targets, want_linear=False, image=True, stream=None):
        """rt_progressive_extend_map_async: trace samples [counts[p], targets[p]) of every pixel p and reduce pixel
        p at targets[p].  Returns what extend() returns."""
        ctx, tp = self.renderer.ctx, _pointer(self._map_argument(targets, "targets"), abi.u32)
        return self._run(lambda rgb, lin: self.lib.rt_progressive_extend_map_async(ctx, tp, rgb, lin, stream),
                         want_linear, image, stream)

    def snapshot(self, counts=None, want_linear=False, stream=None):
        """rt_progressive_snapshot_map_async: the image with pixel p at counts[p] <= its samples so far (None: at
        every pixel's own count), nothing traced.  (rgb, linear | None, RtStats, rc)."""
        c = None if counts is None else self._map_argument(counts, "counts")
        ctx, cp = self.renderer.ctx, _pointer(c, abi.u32)
        return self._run(lambda rgb, lin: self.lib.rt_progressive_snapshot_map_async(ctx, cp, rgb, lin, stream),
                         want_linear, True, stream)

    def error(self, stream=None, stats=False):
        """rt_progressive_error_async: np.float64[n], per pixel the largest channel difference between its linear
        value at counts[p] and at counts[p] // 2 samples; inf below 2 samples.  stats=True: (error, RtStats)."""
        self._require_open()
        lib, ctx = self.lib, self.renderer.ctx
        with abi.DeviceScope(lib, ctx) as dev:
            d_err = dev.alloc(self.npx * 8)
            abi.check(lib, lib.rt_progressive_error_async(ctx, d_err, stream))
            st, _ = abi.collect(lib, ctx, stream, allow_range=True)
            err = dev.download(d_err, np.empty(self.npx, dtype=np.float64))
        return (err, st) if stats else err

    def refine(self, tolerance, spp_max, stream=None):
        """rt_progressive_refine: one step of the doubling policy, selected and planned on the device.  Returns
        (n_active, n_samples): the pixels whose estimate was above `tolerance` and that went to
        min(2 * count, spp_max), and the samples enqueued for them; n_active == 0: converged, nothing traced.  The
        call waits for the selection (one small readback), not for the tracing: collect() follows."""
        self._require_open()
        na, ns = abi.u64(), abi.u64()
        abi.check(self.lib, self.lib.rt_progressive_refine(self.renderer.ctx, float(tolerance), int(spp_max), stream,
                                                           ctypes.byref(na), ctypes.byref(ns)))
        self._stale = True
        return na.value, ns.value

    def refine_items(self):
        """rt_progressive_refine_items: (samples_per_item, items np.uint32[n, 4] of pixel, first, end, 0) of the
        item table the last refine() built on the device; (0, empty) when it selected nothing."""
        self._require_open()
        lib, ctx = self.lib, self.renderer.ctx
        s, n = abi.u32(), abi.u64()
        abi.check(lib, lib.rt_progressive_refine_items(ctx, ctypes.byref(s), ctypes.byref(n), None, 0))
        items = np.zeros((n.value, 4), dtype=np.uint32)
        if n.value:
            abi.check(lib, lib.rt_progressive_refine_items(ctx, ctypes.byref(s), ctypes.byref(n),
                                                           _pointer(items, abi.u32), n.value))
        return s.value, items

    def collect(self, stream=None):
        """rt_context_collect: wait for the work enqueued on `stream` and return its RtStats (a channel above 2.0 in
        one of its reductions is not an error here)."""
        return abi.collect(self.lib, self.renderer.ctx, stream, allow_range=True)[0]

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

    def _use_scene(self, flat):
        """Make flat the context's scene, unless it is already."""
        if self._scene_flat is not flat:
            self.set_scene(flat)

    def render_flat(self, max_bounces, spp, flat, cam, tile_range=None, want_linear=False, samples_per_item=None):
        """Render with a FlatScene / RtCamera; returns (rgb [n,3] u8, linear [n,3] f64 | None, RtStats, rc).
        samples_per_item: None = rt_render_async; 0 = rt_render_split_async with its own plan; n > 0 = that many
        samples per work item (the sample-parallel path, include/rt_mi355x.h)."""
        split = split_argument(samples_per_item)
        self._use_scene(flat)
        tr = _range(cam, tile_range)
        head = (self.ctx, ctypes.byref(cam), max_bounces, spp, self.seed, self.flags, ctypes.byref(tr))

        def launch(d_rgb, d_lin):
            if split is None:
                return self.lib.rt_render_async(*head, d_rgb, d_lin, None)
            return self.lib.rt_render_split_async(*head, d_rgb, d_lin, None, split)

        with abi.DeviceScope(self.lib, self.ctx) as dev:
            return _read_image(dev, tr.row_count * tr.col_count, want_linear, launch)

    def render(self, max_bounces, samples_per_pixel, scene, camera):
        t0 = time.perf_counter()
        cam = _abi_camera(camera)
        rgb, _, st, rc = self.render_flat(max_bounces, samples_per_pixel, _flat(scene), cam,
                                          samples_per_item=0 if self.sample_parallel else None)
        stat = _render_stat(t0, cam, st)
        _raise_range(rc)
        return rgb.reshape(cam.image_height, cam.image_width, 3), stat

    def guides_flat(self, spp, flat, cam, tile_range=None, want=GUIDE_NAMES):
        """rt_render_guides_async with a FlatScene / RtCamera: per pixel the mean first-hit albedo, normal, depth and
        coverage over the primary rays of render_flat's image at `spp` (the renderer's seed and precision; the
        definition is in include/rt_mi355x.h).  Returns ({name: float32 array, flat over the range}, RtStats, rc):
        albedo and normal [n, 3], depth and coverage [n].  want: the buffers to compute the outputs of (a value
        does not depend on which others are asked for)."""
        want = check_guides(self.flags, want)
        self._use_scene(flat)
        tr = _range(cam, tile_range)
        npx = tr.row_count * tr.col_count
        shape = {name: (npx, GUIDE_CHANNELS[name]) if GUIDE_CHANNELS[name] > 1 else (npx,) for name in want}
        with abi.DeviceScope(self.lib, self.ctx) as dev:
            d = {name: dev.alloc(npx * GUIDE_CHANNELS[name] * 4) for name in want}
            abi.check(self.lib, self.lib.rt_render_guides_async(self.ctx, ctypes.byref(cam), spp, self.seed, self.flags,
                                                                ctypes.byref(tr), *[d.get(name) for name in GUIDE_NAMES],
                                                                None))
            st, rc = abi.collect(self.lib, self.ctx)
            out = {name: dev.download(d[name], np.empty(shape[name], dtype=np.float32)) for name in want}
        return out, st, rc

    def guides(self, spp, scene, camera):
        """The guide buffers of render()'s image at `spp` samples: (Guides(albedo (H, W, 3), normal (H, W, 3),
        depth (H, W), coverage (H, W)) of float32, RenderStat).  The means are over all samples of a pixel, so
        they are premultiplied by coverage."""
        check_guides(self.flags)   # before any GPU call
        t0 = time.perf_counter()
        cam = _abi_camera(camera)
        out, st, _ = self.guides_flat(spp, _flat(scene), cam)
        stat = _render_stat(t0, cam, st)
        h, w = cam.image_height, cam.image_width
        return Guides(out["albedo"].reshape(h, w, 3), out["normal"].reshape(h, w, 3), out["depth"].reshape(h, w),
                      out["coverage"].reshape(h, w)), stat

    def _query_flags(self, root2):
        return self.flags | (abi.RT_FLAG_ROOT2 if root2 else 0)

    def _launch_query(self, n, d_org, origin, d_dir, flags, ptrs, stream):
        return self.lib.rt_query_hits_async(self.ctx, n, d_org, _pointer(origin, abi.f64), d_dir, flags,
                                            *[ptrs.get(name) for name in QUERY_NAMES], stream)

    def _launch_rays(self, n, spp, R, d_org, origin, d_dir, max_bounces, seed, pixel_base, flags, d_rgb, d_lin, stream):
        return self.lib.rt_render_rays_async(self.ctx, n, spp, R, d_org, _pointer(origin, abi.f64), d_dir, max_bounces,
                                             self.seed if seed is None else seed, pixel_base, flags, d_rgb, d_lin, stream)

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
        out = {name: np.empty(_query_shape(name, n), dtype=QUERY_OUTPUTS[name][1] or d.dtype) for name in want}
        self._use_scene(_flat(scene))
        if n == 0:
            self.query_stats = abi.RtStats()
            return out
        with abi.DeviceScope(self.lib, self.ctx) as dev:
            d_dir = dev.upload(d)
            d_org = None if shared else dev.upload(o)
            ptrs = {name: dev.alloc(out[name].nbytes) for name in want}
            abi.check(self.lib, self._launch_query(n, d_org, o if shared else None, d_dir, flags, ptrs, None))
            self.query_stats, _ = abi.collect(self.lib, self.ctx)
            for name in want:
                dev.download(ptrs[name], out[name])
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
        check_stream(stream)
        if self._scene_flat is None:
            raise RuntimeError("query_into needs a scene: call set_scene first")
        abi.check(self.lib, self._launch_query(n, d_org, origin, d_dir, flags, ptrs, stream))
        return n

    def _launch_occluded(self, n, d_org, origin, d_dir, d_t_max, t_max, flags, d_occ, stream):
        return self.lib.rt_query_occluded_async(self.ctx, n, d_org, _pointer(origin, abi.f64), d_dir, d_t_max, t_max,
                                                flags, d_occ, stream)

    def occluded(self, origins, directions, scene, t_max=np.inf, root2=False):
        """rt_query_occluded_async with numpy arrays: is anything in the way of each ray before its t_max
        (include/rt_mi355x.h has the definition).  directions: (n, 3), not normalised, so d = light - p with t_max = 1
        asks about the open segment up to the light; origins: (n, 3), or (3,) for one shared origin; t_max: a number
        (not NaN; the default +inf: unbounded) or an (n,) array, one bound per ray.  The arrays are converted to the
        renderer's precision.  root2: quirk Q1 off, as in query().
        Returns uint8 (n,): abi.RT_OCCLUDED_NO = 0, abi.RT_OCCLUDED_YES = 1 (an accepted root r < t_max, strictly),
        abi.RT_OCCLUDED_INVALID = 255 (a ray outside query()'s precondition or with a NaN t_max: not traced).  The
        call's RtStats are kept in self.query_stats."""
        flags = self._query_flags(root2)
        o, d, shared, t = check_occluded(flags, origins, directions, t_max)   # before any GPU call
        n = d.shape[0]
        out = np.empty(n, dtype=np.uint8)
        self._use_scene(_flat(scene))
        if n == 0:
            self.query_stats = abi.RtStats()
            return out
        with abi.DeviceScope(self.lib, self.ctx) as dev:
            d_dir = dev.upload(d)
            d_org = None if shared else dev.upload(o)
            per_ray = isinstance(t, np.ndarray)
            d_t = dev.upload(t) if per_ray else None
            d_occ = dev.alloc(out.nbytes)
            abi.check(self.lib, self._launch_occluded(n, d_org, o if shared else None, d_dir, d_t, 0.0 if per_ray else t,
                                                      flags, d_occ, None))
            self.query_stats, _ = abi.collect(self.lib, self.ctx)
            dev.download(d_occ, out)
        return out

    def occluded_into(self, origins, directions, occluded, *, t_max=np.inf, stream=None, root2=False):
        """rt_query_occluded_async on device arrays in place, without a copy: directions (n, 3) in the renderer's
        precision and occluded (n,) uint8 are objects exposing __cuda_array_interface__ (torch ROCm tensors do),
        C-contiguous, on the renderer's device.  origins: such an array of shape (n, 3), or 3 host numbers for one
        shared origin.  t_max: a number (not NaN), or such an array of shape (n,) in the renderer's precision.  The
        scene is the one last set (set_scene); stream as in query_into.  Returns the number of rays."""
        flags = self._query_flags(root2)
        n, d_org, origin, d_dir, d_t, t, d_occ = check_occluded_into(flags, self.device, origins, directions, occluded, t_max)
        check_stream(stream)
        check_scene_set(self._scene_flat)
        abi.check(self.lib, self._launch_occluded(n, d_org, origin, d_dir, d_t, t, flags, d_occ, stream))
        return n

    def _launch_scatter(self, n, d_org, origin, d_dir, d_idx, d_t, d_pix, d_smp, bounce, seed, flags, d_col, d_oo, d_od,
                        stream):
        return self.lib.rt_scatter_async(self.ctx, n, d_org, _pointer(origin, abi.f64), d_dir, d_idx, d_t, d_pix, d_smp,
                                         bounce, self.seed if seed is None else seed, flags, d_col, d_oo, d_od, stream)

    def _launch_step(self, n, d_org, d_dir, d_col, d_pix, d_smp, bounce, seed, flags, ptrs, stream):
        return self.lib.rt_path_step_async(self.ctx, n, d_org, d_dir, d_col, d_pix, d_smp, bounce,
                                           self.seed if seed is None else seed, flags,
                                           *[ptrs.get(name) for name in STEP_NAMES], stream)

    def scatter(self, origins, directions, index, t, scene, pixel=None, sample=None, bounce=0, colour=None, seed=None,
                root2=False):
        """rt_scatter_async with numpy arrays: the material stage of a render for rays whose hits are known
        (include/rt_mi355x.h has the definition).  origins, directions: as query() takes them; index, t: as query()
        returns them; pixel, sample: (n,) integers, the counter of each ray's draw (None: arange(n) and zeros); bounce:
        the draw's bounce; colour: (n, 3) or None; seed: the RNG key (None: the renderer's).
        Returns {"origins": (n, 3), "directions": (n, 3), "colour": (n, 3) | None}: a ray with index >= 0 as its
        scattered ray (origin the hit point, direction not normalised, colour times the attenuation), any other ray as
        it came.  The call's RtStats are kept in self.query_stats."""
        flags = self._query_flags(root2)
        o, d, shared, i, tt, pix, smp, col, bounce = check_scatter(flags, origins, directions, index, t, pixel, sample,
                                                                    colour, bounce)   # before any GPU call
        seed = check_seed(seed)
        n = d.shape[0]
        out = {"origins": np.empty((n, 3), dtype=d.dtype), "directions": np.empty((n, 3), dtype=d.dtype), "colour": col}
        self._use_scene(_flat(scene))
        if n == 0:
            self.query_stats = abi.RtStats()
            return out
        with abi.DeviceScope(self.lib, self.ctx) as dev:
            d_dir = dev.upload(d)
            d_org = None if shared else dev.upload(o)
            d_col = None if col is None else dev.upload(col)
            d_oo = dev.alloc(d.nbytes) if shared else d_org
            abi.check(self.lib, self._launch_scatter(n, d_org, o if shared else None, d_dir, dev.upload(i), dev.upload(tt),
                                                     dev.upload(pix), dev.upload(smp), bounce, seed, flags, d_col, d_oo,
                                                     d_dir, None))
            self.query_stats, _ = abi.collect(self.lib, self.ctx)
            dev.download(d_oo, out["origins"])
            dev.download(d_dir, out["directions"])
            if col is not None:
                dev.download(d_col, col)
        return out

    def scatter_into(self, origins, directions, index, t, pixel, sample, *, bounce=0, colour=None, out_origins=None,
                     out_directions=None, seed=None, stream=None, root2=False):
        """rt_scatter_async on device arrays, without a copy: directions (n, 3), index (n,) int32, t (n,), pixel and
        sample (n,) uint32 and colour (n, 3) (or None) are objects exposing __cuda_array_interface__ (torch ROCm tensors
        do), C-contiguous, on the renderer's device, the reals in the renderer's precision.  origins: such an array of
        shape (n, 3), or 3 host numbers for one shared origin.  out_origins, out_directions: where the scattered rays
        go; None: in place (with a shared origin: out_origins = None writes no origins).  colour is updated in place.
        The scene is the one last set (set_scene); stream as in query_into.  Returns the number of rays."""
        flags = self._query_flags(root2)
        n, d_org, origin, d_dir, d_idx, d_t, d_pix, d_smp, d_col, d_oo, d_od, bounce = check_scatter_into(
            flags, self.device, origins, directions, index, t, pixel, sample, colour, out_origins, out_directions, bounce)
        seed = check_seed(seed)
        check_stream(stream)
        check_step_scene(self._scene_flat, "scatter_into")
        abi.check(self.lib, self._launch_scatter(n, d_org, origin, d_dir, d_idx, d_t, d_pix, d_smp, bounce, seed, flags,
                                                 d_col, d_oo, d_od, stream))
        return n

    def path_step(self, origins, directions, scene, pixel=None, sample=None, bounce=0, colour=None, seed=None,
                  root2=False, want=STEP_NAMES):
        """rt_path_step_async with numpy arrays: the closest hit of each ray and its scatter in one kernel
        (include/rt_mi355x.h has the definition).  origins, directions: (n, 3); pixel, sample, bounce, colour, seed as in
        scatter().  Returns a dict: "origins", "directions" (n, 3) and "colour" ((n, 3) | None) after the step (a hit as
        its scattered ray; a miss and an invalid ray as they came), and for the names in `want`: status (n,) uint8
        (abi.RT_STEP_SCATTERED, RT_STEP_MISSED, RT_STEP_INVALID) and the query's index, t, normal and front of the hit
        that was scattered.  The call's RtStats are kept in self.query_stats."""
        flags = self._query_flags(root2)
        o, d, pix, smp, col, bounce = check_path_step(flags, origins, directions, pixel, sample, colour, bounce)
        seed = check_seed(seed)
        want = check_step_names(want)
        n = d.shape[0]
        out = {"origins": o, "directions": d, "colour": col}
        out.update({name: np.empty(_step_shape(name, n), dtype=STEP_OUTPUTS[name][1] or d.dtype) for name in want})
        self._use_scene(_flat(scene))
        if n == 0:
            self.query_stats = abi.RtStats()
            return out
        with abi.DeviceScope(self.lib, self.ctx) as dev:
            d_org, d_dir = dev.upload(o), dev.upload(d)
            d_col = None if col is None else dev.upload(col)
            ptrs = {name: dev.alloc(out[name].nbytes) for name in want}
            abi.check(self.lib, self._launch_step(n, d_org, d_dir, d_col, dev.upload(pix), dev.upload(smp), bounce, seed,
                                                  flags, ptrs, None))
            self.query_stats, _ = abi.collect(self.lib, self.ctx)
            dev.download(d_org, o)
            dev.download(d_dir, d)
            if col is not None:
                dev.download(d_col, col)
            for name in want:
                dev.download(ptrs[name], out[name])
        return out

    def path_step_into(self, origins, directions, pixel, sample, *, bounce=0, colour=None, status=None, index=None,
                       t=None, normal=None, front=None, seed=None, stream=None, root2=False):
        """rt_path_step_async on device arrays in place, without a copy: origins and directions (n, 3) and colour
        (n, 3) (or None) are updated; pixel and sample are (n,) uint32; status (n,) uint8, index (n,) int32, t (n,),
        normal (n, 3) and front (n,) uint8 are optional outputs.  All are objects exposing __cuda_array_interface__
        (torch ROCm tensors do), C-contiguous, on the renderer's device, the reals in the renderer's precision.  The
        scene is the one last set (set_scene); stream as in query_into.  Returns the number of rays."""
        flags = self._query_flags(root2)
        n, d_org, d_dir, d_col, d_pix, d_smp, ptrs, bounce = check_path_step_into(
            flags, self.device, origins, directions, pixel, sample, colour,
            dict(status=status, index=index, t=t, normal=normal, front=front), bounce)
        seed = check_seed(seed)
        check_stream(stream)
        check_step_scene(self._scene_flat, "path_step_into")
        abi.check(self.lib, self._launch_step(n, d_org, d_dir, d_col, d_pix, d_smp, bounce, seed, flags, ptrs, stream))
        return n

    def path_step_list_into(self, origins, directions, pixel, sample, *, bounce, list_in=None, count_in=None,
                            list_out=None, count_out=None, colour=None, status=None, index=None, t=None, normal=None,
                            front=None, seed=None, root2=False, stream=None):
        """rt_path_step_list_async on device arrays in place: path_step_into over the rays a list names, leaving the
        next list on the device (include/rt_mi355x.h has the definition).  The ray arrays are path_step_into's, indexed
        by ray id; list_in (n,) uint32 and count_in (1,) uint32 name the rays (None: the identity list, count n);
        list_out (n,) uint32 and count_out (1,) uint32, given together, receive the rays that scattered, in list
        order.  Nothing is written at a ray that is not listed.  Returns the number of rays n (the capacity)."""
        flags = self._query_flags(root2)
        n, d_org, d_dir, d_col, d_pix, d_smp, ptrs, bounce, lists = check_path_step_list_into(
            flags, self.device, origins, directions, pixel, sample, colour,
            dict(status=status, index=index, t=t, normal=normal, front=front), bounce, list_in, count_in, list_out, count_out)
        seed = check_seed(seed)
        check_stream(stream)
        check_step_scene(self._scene_flat, "path_step_list_into")
        d_li, d_ci, d_lo, d_co = lists
        abi.check(self.lib, self.lib.rt_path_step_list_async(
            self.ctx, n, d_li, d_ci, d_org, d_dir, d_col, d_pix, d_smp, bounce, self.seed if seed is None else seed, flags,
            *[ptrs.get(name) for name in STEP_NAMES], d_lo, d_co, stream))
        return n

    def compact_list_into(self, keep, list_out, count_out, *, list_in=None, count_in=None, stream=None):
        """rt_ray_list_compact_async on device arrays: list_out receives, in list order, the entries r of list_in
        (None: 0 .. n - 1; count_in None: all n) with keep[r] != 0, and count_out how many.  keep: (n,) uint8 by ray id
        (a step's status array builds a list of the scattered and invalid rays).  Returns n."""
        n, d_keep, (d_li, d_ci, d_lo, d_co) = check_compact_list_into(self.device, keep, list_out, count_out, list_in, count_in)
        check_stream(stream)
        abi.check(self.lib, self.lib.rt_ray_list_compact_async(self.ctx, n, d_li, d_ci, d_keep, d_lo, d_co, stream))
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
        self._use_scene(_flat(scene))
        if n == 0:
            return (np.empty((0, 3), dtype=np.uint8), np.empty((0, 3), dtype=np.float64) if want_linear else None,
                    abi.RtStats(), abi.RT_OK)
        with abi.DeviceScope(self.lib, self.ctx) as dev:
            d_dir = dev.upload(d)
            d_org = None if shared else dev.upload(o)
            return _read_image(dev, n, want_linear, lambda d_rgb, d_lin: self._launch_rays(
                n, spp, R, d_org, o if shared else None, d_dir, max_bounces, seed, pixel_base, flags, d_rgb, d_lin, None))

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
        check_stream(stream)
        if self._scene_flat is None:
            raise RuntimeError("render_rays_into needs a scene: call set_scene first")
        abi.check(self.lib, self._launch_rays(n, spp, R, d_org, origin, d_dir, max_bounces, seed, pixel_base, flags,
                                              d_rgb, d_lin, stream))
        return n

    def begin_progressive(self, max_bounces, spp_capacity, scene, camera, tile_range=None, max_bytes=0):
        """Open a ProgressiveSession (rt_progressive_begin) for up to spp_capacity samples per pixel.  The live
        path only: mode "vectorized2" without root2.  max_bytes: the most the record buffer may take
        (0 = the library's 24 GB budget; see rt_progressive_bytes for the cost)."""
        return ProgressiveSession(self, max_bounces, spp_capacity, _flat(scene), _abi_camera(camera), tile_range,
                                  max_bytes)

    def progressive(self, max_bounces, schedule, scene, camera):
        """Render at each sample count of `schedule` (strictly increasing), tracing only the new samples of
        each step: yields (spp, image HxWx3 uint8, RenderStat) per step, every image equal to render()'s at
        that spp.  A step whose image has a channel above 2.0 (RT_ERR_RANGE; at 1 spp the reference's own
        arithmetic gets there) is yielded with stat.range_error set instead of raising, so that a preview
        never aborts the run.  The stat's samples and ray_segments are those of the step."""
        counts = check_schedule(schedule)   # before any GPU call
        return self._progressive(max_bounces, counts, scene, camera)

    def _progressive(self, max_bounces, counts, scene, camera):
        cam = _abi_camera(camera)
        with self.begin_progressive(max_bounces, counts[-1], scene, cam) as session:
            for n in counts:
                t0 = time.perf_counter()
                rgb, _, st, rc = session.extend(n)
                stat = _render_stat(t0, cam, st, range_error=rc == abi.RT_ERR_RANGE)
                yield n, rgb.reshape(cam.image_height, cam.image_width, 3), stat

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
        cam = _abi_camera(camera)
        total = abi.RtStats()   # the work counters summed over the run

        def add(st):
            for field in ("kernel_ms", "samples", "ray_segments", "bounce_iters"):
                setattr(total, field, getattr(total, field) + getattr(st, field))

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
        stat = _render_stat(t0, cam, total, bounce_iters=total.bounce_iters)
        _raise_range(rc)
        h, w = cam.image_height, cam.image_width
        return rgb.reshape(h, w, 3), counts.reshape(h, w), stat
