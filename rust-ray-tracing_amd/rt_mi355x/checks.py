"""Argument checks of the Python layer: everything that runs before any GPU call and needs no library.

renderer.py re-exports every public name here.  The ray checks come in pairs (a query and a caller-ray render take
the same rays, a render with one more rank); each pair is one implementation with the pair's ranks and texts.
"""
import collections

import numpy as np

from . import abi

ADAPTIVE_PLANS = ("host", "device")

# Guide buffers (rt_render_guides_async), in the C ABI's argument order, and their channels per pixel.
GUIDE_NAMES = ("albedo", "normal", "depth", "coverage")
GUIDE_CHANNELS = {"albedo": 3, "normal": 3, "depth": 1, "coverage": 1}
Guides = collections.namedtuple("Guides", GUIDE_NAMES)

# Ray-query outputs (rt_query_hits_async), in the C ABI's argument order: name -> (components per ray, dtype; None:
# the rays' precision).
QUERY_NAMES = ("t", "index", "normal", "point", "front")
QUERY_OUTPUTS = {"t": (1, None), "index": (1, np.int32), "normal": (3, None), "point": (3, None), "front": (1, np.uint8)}

# What differs between the two users of the ray checks: the ranks of `directions`, that shape in words, the shape a
# device `origins` has in words, and the refusal of any flag but the live path's.
RaySpec = collections.namedtuple("RaySpec", "ranks shape origins refusal")
LIVE_PATH = abi.RT_FLAG_F32 | abi.RT_FLAG_ROOT2
QUERY_RAYS = RaySpec((2,), "(n, 3)", "of shape (n, 3)",
                     "ray queries are the live path's closest hit: mode 'vectorized2' only (root2 is allowed)")
RENDER_RAYS = RaySpec((2, 3), "(n, R, 3) or (n, 3)", "shaped like directions",
                      "caller rays are rendered on the live path: mode 'vectorized2' only (root2 is allowed)")


def _is_int(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def _live_path(flags, allowed, refusal):
    """The live path's flags only (no mode flag; root2 where `allowed` has it).  Returns the rays' precision."""
    if flags & ~allowed:
        raise ValueError(refusal)
    return np.dtype(np.float32 if flags & abi.RT_FLAG_F32 else np.float64)


def _known_names(want, names, what):
    want = tuple(want)
    for name in want:
        if name not in names:
            raise ValueError(f"unknown {what} {name!r} (one of {list(names)})")
    if not want:
        raise ValueError(f"no {what} asked for")
    return want


def check_stream(stream):
    """A stream argument: an integer handle (a plain int, as torch's .cuda_stream is) or None."""
    if stream is not None and (isinstance(stream, bool) or not isinstance(stream, int)):
        raise TypeError(f"stream must be an integer stream handle or None, not {stream!r}")


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
        if not _is_int(n):
            raise ValueError(f"progressive schedule entries must be ints, not {n!r}")
    counts = [int(n) for n in counts]
    if counts[0] < 1:
        raise ValueError(f"progressive schedule must start at 1 sample or more, not {counts[0]}")
    for a, b in zip(counts, counts[1:]):
        if b <= a:
            raise ValueError(f"progressive schedule must be strictly increasing ({a} is followed by {b})")
    return counts


def check_adaptive(spp_min, spp_max, tolerance, plan="host"):
    """GpuRenderer.adaptive's arguments checked before any GPU call: 1 <= spp_min <= spp_max, a tolerance that is
    a number (not NaN), a plan that is "host" or "device".  Returns (spp_min, spp_max, tolerance) as
    (int, int, float)."""
    if plan not in ADAPTIVE_PLANS:
        raise ValueError(f"unknown plan {plan!r} (one of {list(ADAPTIVE_PLANS)})")
    for name, n in (("spp_min", spp_min), ("spp_max", spp_max)):
        if not _is_int(n):
            raise ValueError(f"{name} must be an int, not {n!r}")
    if spp_min < 1:
        raise ValueError(f"spp_min must be 1 or more, not {spp_min}")
    if spp_min > spp_max:
        raise ValueError(f"spp_min ({spp_min}) is above spp_max ({spp_max})")
    tolerance = float(tolerance)
    if tolerance != tolerance:
        raise ValueError("tolerance is NaN")
    return int(spp_min), int(spp_max), tolerance


def check_guides(flags, want=GUIDE_NAMES):
    """The guide calls' arguments checked before any GPU call: the live path only, known output names."""
    _live_path(flags, abi.RT_FLAG_F32, "guide buffers are the live path's first hits: mode 'vectorized2' without root2 only")
    return _known_names(want, GUIDE_NAMES, "guide buffer")


def _query_shape(name, n):
    return (n, 3) if QUERY_OUTPUTS[name][0] == 3 else (n,)


def _query_count(n, R):
    if n > 0x7FFFFFFF:
        raise ValueError("more than 0x7FFFFFFF rays in one query")


def _rays_counts(spp, n, R, pixel_base):
    if not _is_int(spp) or not 1 <= spp <= 1 << 20:
        raise ValueError(f"spp must be an integer in 1..2^20, not {spp!r}")
    if not 1 <= R <= spp:
        raise ValueError(f"rays per pixel must be within 1..spp: directions has {R} rays per pixel, spp is {spp}")
    if n > 0x7FFFFFFF:
        raise ValueError("more than 0x7FFFFFFF pixels in one call")
    if not _is_int(pixel_base) or pixel_base < 0 or pixel_base + n > 1 << 32:
        raise ValueError(f"pixel_base must be an integer with pixel_base + n <= 2^32, not {pixel_base!r}")


def _host_rays(dtype, origins, directions, rays, counts):
    """Rays in host arrays: directions of one of the ranks of `rays` with 3 components last, origins the same shape
    or (3,) for one shared origin, of finite-or-not numbers (the library judges each ray); counts(n, R) judges the
    counts before anything is copied.  Returns (origins, directions, shared), the arrays contiguous in `dtype`, a
    shared origin kept in float64 (the library rounds it the way it rounds a camera centre)."""
    d = np.asarray(directions)
    o = np.asarray(origins)
    for what, a in (("directions", d), ("origins", o)):
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{what} must be numbers, not dtype {a.dtype}")
    if d.ndim not in rays.ranks or d.shape[-1] != 3:
        raise ValueError(f"directions must have shape {rays.shape}, not {d.shape}")
    shared = o.shape == (3,)
    if not shared and o.shape != d.shape:
        raise ValueError(f"origins must have shape (3,) (one shared origin) or {d.shape} like directions, not {o.shape}")
    counts(d.shape[0], d.shape[1] if d.ndim == 3 else 1)
    o = np.ascontiguousarray(o, dtype=np.float64 if shared else dtype)
    return o, np.ascontiguousarray(d, dtype=dtype), shared


def check_query(flags, origins, directions, want=QUERY_NAMES):
    """GpuRenderer.query's arguments checked before any GPU call: the live path's hit only (no mode flag), known
    output names, directions (n, 3) and origins (n, 3) or (3,).  Returns (origins, directions, shared, want) with
    the arrays contiguous in the renderer's precision; shared: origins has shape (3,) and is kept in float64."""
    dtype = _live_path(flags, LIVE_PATH, QUERY_RAYS.refusal)
    want = _known_names(want, QUERY_NAMES, "query output")
    return _host_rays(dtype, origins, directions, QUERY_RAYS, _query_count) + (want,)


def check_render_rays(flags, spp, origins, directions, pixel_base=0):
    """GpuRenderer.render_rays' arguments checked before any GPU call.  directions: (n, R, 3) or (n, 3) (R = 1);
    origins: the same shape, or (3,) for one shared origin.  Returns (origins, directions (n, R, 3), shared), the arrays
    contiguous in the renderer's precision, a shared origin kept in float64."""
    o, d, shared = _host_rays(_live_path(flags, LIVE_PATH, RENDER_RAYS.refusal), origins, directions, RENDER_RAYS,
                              lambda n, R: _rays_counts(spp, n, R, pixel_base))
    d = d.reshape(d.shape[0], d.shape[1] if d.ndim == 3 else 1, 3)
    return o if shared else o.reshape(d.shape), d, shared


def _device_array(obj, what, dtype, shape, device):
    """The device pointer of obj, an object exposing __cuda_array_interface__ (a torch ROCm tensor does), after
    checking dtype, shape, contiguity and, where the object names one (torch's .device), the device."""
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


def _device_output(obj, name, dtype, shape, device):
    """_device_array of an output: not read-only."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if isinstance(cai, dict) and cai["data"][1]:
        raise ValueError(f"{name} is read-only")
    return _device_array(obj, name, dtype, shape, device)


def _device_rays(dtype, device, origins, directions, rays, counts):
    """Rays in device arrays: directions of one of the ranks of `rays`, origins a device array of the same shape or 3
    host numbers for one shared origin; counts(n, R) judges the counts.  Returns (n, R, d_origins | None,
    origin | None, d_directions)."""
    cai = getattr(directions, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError(f"directions must expose __cuda_array_interface__ (a device array), not {type(directions).__name__}")
    shape = tuple(cai["shape"])
    if len(shape) not in rays.ranks or shape[-1] != 3:
        raise ValueError(f"directions must have shape {rays.shape}, not {shape}")
    n, R = shape[0], (shape[1] if len(shape) == 3 else 1)
    counts(n, R)
    d_dir = _device_array(directions, "directions", dtype, shape, device)
    d_org, origin = None, None
    if hasattr(origins, "__cuda_array_interface__"):
        d_org = _device_array(origins, "origins", dtype, shape, device)
    else:
        origin = np.asarray(origins)
        if origin.shape != (3,) or origin.dtype.kind not in "fiu":
            raise ValueError(f"origins must be a device array {rays.origins} or one shared origin of 3 host numbers")
        origin = np.ascontiguousarray(origin, dtype=np.float64)
    return n, R, d_org, origin, d_dir


def check_query_into(flags, device, origins, directions, outputs):
    """GpuRenderer.query_into's arguments checked before any GPU call.  Returns (n, d_origins | None, origin | None,
    d_directions, {name: pointer})."""
    dtype = _live_path(flags, LIVE_PATH, QUERY_RAYS.refusal)
    n, _, d_org, origin, d_dir = _device_rays(dtype, device, origins, directions, QUERY_RAYS, _query_count)
    ptrs = {name: _device_output(obj, name, QUERY_OUTPUTS[name][1] or dtype, _query_shape(name, n), device)
            for name, obj in outputs.items() if obj is not None}
    if not ptrs:
        raise ValueError("no query output given")
    return n, d_org, origin, d_dir, ptrs


def check_render_rays_into(flags, device, spp, origins, directions, rgb, linear, pixel_base=0):
    """GpuRenderer.render_rays_into's arguments checked before any GPU call.  Returns (n, R, d_origins | None,
    origin | None, d_directions, d_rgb | None, d_linear | None)."""
    rays = _device_rays(_live_path(flags, LIVE_PATH, RENDER_RAYS.refusal), device, origins, directions, RENDER_RAYS,
                        lambda n, R: _rays_counts(spp, n, R, pixel_base))
    d_rgb, d_lin = (None if obj is None else _device_output(obj, name, dt, (rays[0], 3), device)
                    for name, obj, dt in (("rgb", rgb, np.uint8), ("linear", linear, np.float64)))
    if d_rgb is None and d_lin is None:
        raise ValueError("no output given (rgb or linear)")
    return rays + (d_rgb, d_lin)
