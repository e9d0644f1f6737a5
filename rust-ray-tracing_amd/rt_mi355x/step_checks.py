"""Argument checks of the path steps (GpuRenderer.scatter, scatter_into, path_step, path_step_into): everything that
runs before any GPU call and needs no library.  The ray checks are checks.py's, the ones a ray query takes, reused and
not copied; what is added here is the hit (index, t), the draw's counter (pixel, sample, bounce), the colour and the
outputs.
"""
import numpy as np

from . import abi
from .checks import (LIVE_PATH, QUERY_OUTPUTS, QUERY_RAYS, _device_array, _device_output, _device_rays, _host_rays,
                     _is_int, _live_path, _query_count, _query_shape)

STEP_REFUSAL = "path steps scatter on the live path: mode 'vectorized2' only (root2 is allowed)"

# The fused step's outputs beside the rays and the colour, in the C ABI's argument order.
STEP_NAMES = ("status", "index", "t", "normal", "front")
STEP_OUTPUTS = dict(QUERY_OUTPUTS, status=(1, np.uint8))


STEP_RAYS = QUERY_RAYS._replace(refusal=STEP_REFUSAL)


def _step_shape(name, n):
    return (n,) if name == "status" else _query_shape(name, n)


def check_step_names(want):
    """path_step's `want`: names of STEP_NAMES, possibly none (the rays and the colour always come back)."""
    want = tuple(want)
    for name in want:
        if name not in STEP_NAMES:
            raise ValueError(f"unknown path-step output {name!r} (one of {list(STEP_NAMES)})")
    return want


def check_bounce(flags, bounce):
    """The bounce of the draw: an integer in 0..2^32 - 1, in fp32 at most RT_MAX_BOUNCES_F32 (the library refuses more)."""
    if not _is_int(bounce) or not 0 <= bounce < 1 << 32:
        raise ValueError(f"bounce must be an integer in 0..2^32 - 1, not {bounce!r}")
    if flags & abi.RT_FLAG_F32 and bounce > abi.RT_MAX_BOUNCES_F32:
        raise ValueError(f"an fp32 renderer scatters bounces 0..{abi.RT_MAX_BOUNCES_F32} only, not {bounce}")
    return int(bounce)


def check_seed(seed):
    """The RNG key of a step: None (the renderer's seed) or an integer in 0..2^64 - 1."""
    if seed is None:
        return None
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in 0..2^64 - 1 or None, not {seed!r}")
    return int(seed)


def _host_u32(a, what, n, default):
    """pixel / sample: None (the default), or n integers in 0..2^32 - 1.  Returns a contiguous uint32 array."""
    if a is None:
        return default(n)
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be integers, not dtype {a.dtype}")
    if a.shape != (n,):
        raise ValueError(f"{what} must have shape ({n},), one per ray, not {a.shape}")
    if a.size and (a.min() < 0 or a.max() >= 1 << 32):
        raise ValueError(f"{what} must lie in 0..2^32 - 1")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _default_pixel(n):
    return np.arange(n, dtype=np.uint32)


def _default_sample(n):
    return np.zeros(n, dtype=np.uint32)


def _host_colour(colour, dtype, n):
    if colour is None:
        return None
    c = np.asarray(colour)
    if c.dtype.kind not in "fiu":
        raise ValueError(f"colour must be numbers, not dtype {c.dtype}")
    if c.shape != (n, 3):
        raise ValueError(f"colour must have shape ({n}, 3), one per ray, not {c.shape}")
    return np.array(c, dtype=dtype, order="C")   # a copy: the call updates it


def check_scatter(flags, origins, directions, index, t, pixel=None, sample=None, colour=None, bounce=0):
    """GpuRenderer.scatter's arguments checked before any GPU call: a query's rays, index (n,) integers and t (n,)
    numbers as query() returns them, pixel and sample (n,) integers or None (arange(n) and zeros), colour (n, 3) or
    None.  Returns (origins, directions, shared, index, t, pixel, sample, colour | None, bounce), the arrays contiguous
    in the renderer's precision (index int32, pixel and sample uint32), a shared origin kept in float64."""
    dtype = _live_path(flags, LIVE_PATH, STEP_REFUSAL)
    bounce = check_bounce(flags, bounce)
    o, d, shared = _host_rays(dtype, origins, directions, STEP_RAYS, _query_count)
    n = d.shape[0]
    i = np.asarray(index)
    if i.dtype.kind not in "iu" or i.shape != (n,):
        raise ValueError(f"index must be ({n},) integers, a query's index, not {i.dtype} {i.shape}")
    if i.size and (i.min() < -(1 << 31) or i.max() >= 1 << 31):
        raise ValueError("index must fit int32")
    tt = np.asarray(t)
    if tt.dtype.kind not in "fiu" or tt.shape != (n,):
        raise ValueError(f"t must be ({n},) numbers, a query's t, not {tt.dtype} {tt.shape}")
    return (o, d, shared, np.ascontiguousarray(i, dtype=np.int32), np.ascontiguousarray(tt, dtype=dtype),
            _host_u32(pixel, "pixel", n, _default_pixel), _host_u32(sample, "sample", n, _default_sample),
            _host_colour(colour, dtype, n), bounce)


def check_path_step(flags, origins, directions, pixel=None, sample=None, colour=None, bounce=0):
    """GpuRenderer.path_step's arguments checked before any GPU call: origins and directions (n, 3) (no shared origin:
    the step writes the origins back), pixel, sample and colour as check_scatter has them.  Returns (origins, directions,
    pixel, sample, colour | None, bounce); the arrays are copies the call may update."""
    dtype = _live_path(flags, LIVE_PATH, STEP_REFUSAL)
    bounce = check_bounce(flags, bounce)
    if np.shape(origins) != np.shape(directions):
        raise ValueError(f"origins must have the shape of directions, one per ray (the step writes them back), "
                         f"not {np.shape(origins)}")
    o, d, _ = _host_rays(dtype, origins, directions, STEP_RAYS, _query_count)
    n = d.shape[0]
    return (np.array(o, dtype=dtype, order="C"), np.array(d, dtype=dtype, order="C"),
            _host_u32(pixel, "pixel", n, _default_pixel), _host_u32(sample, "sample", n, _default_sample),
            _host_colour(colour, dtype, n), bounce)


def _device_counter(device, n, pixel, sample):
    return (_device_array(pixel, "pixel", np.uint32, (n,), device), _device_array(sample, "sample", np.uint32, (n,), device))


def check_scatter_into(flags, device, origins, directions, index, t, pixel, sample, colour, out_origins, out_directions,
                       bounce=0):
    """GpuRenderer.scatter_into's arguments checked before any GPU call: device arrays throughout (origins may be 3
    host numbers).  out_origins / out_directions: None (in place where the input is a device array, else not written)
    or a writable device array (n, 3).  Returns (n, d_origins | None, origin | None, d_directions, d_index, d_t, d_pixel,
    d_sample, d_colour | None, d_out_origins | None, d_out_directions, bounce)."""
    dtype = _live_path(flags, LIVE_PATH, STEP_REFUSAL)
    bounce = check_bounce(flags, bounce)
    n, _, d_org, origin, d_dir = _device_rays(dtype, device, origins, directions, STEP_RAYS, _query_count)
    d_idx = _device_array(index, "index", np.int32, (n,), device)
    d_t = _device_array(t, "t", dtype, (n,), device)
    d_pix, d_smp = _device_counter(device, n, pixel, sample)
    d_col = None if colour is None else _device_output(colour, "colour", dtype, (n, 3), device)
    if out_origins is not None:
        d_oo = _device_output(out_origins, "out_origins", dtype, (n, 3), device)
    else:
        d_oo = None if d_org is None else _device_output(origins, "origins", dtype, (n, 3), device)
    if out_directions is not None:
        d_od = _device_output(out_directions, "out_directions", dtype, (n, 3), device)
    else:
        d_od = _device_output(directions, "directions", dtype, (n, 3), device)
    return n, d_org, origin, d_dir, d_idx, d_t, d_pix, d_smp, d_col, d_oo, d_od, bounce


def check_path_step_into(flags, device, origins, directions, pixel, sample, colour, outputs, bounce=0):
    """GpuRenderer.path_step_into's arguments checked before any GPU call: origins and directions writable device
    arrays (n, 3), pixel and sample device arrays (n,) uint32, colour a writable device array (n, 3) or None, outputs
    {name: device array | None} over STEP_NAMES.  Returns (n, d_origins, d_directions, d_colour | None, d_pixel,
    d_sample, {name: pointer}, bounce)."""
    dtype = _live_path(flags, LIVE_PATH, STEP_REFUSAL)
    bounce = check_bounce(flags, bounce)
    if not hasattr(origins, "__cuda_array_interface__"):
        raise TypeError("origins must be a device array of shape (n, 3): the step writes the origins back")
    n, _, _, _, _ = _device_rays(dtype, device, origins, directions, STEP_RAYS, _query_count)
    d_org = _device_output(origins, "origins", dtype, (n, 3), device)
    d_dir = _device_output(directions, "directions", dtype, (n, 3), device)
    d_pix, d_smp = _device_counter(device, n, pixel, sample)
    d_col = None if colour is None else _device_output(colour, "colour", dtype, (n, 3), device)
    ptrs = {name: _device_output(obj, name, STEP_OUTPUTS[name][1] or dtype, _step_shape(name, n), device)
            for name, obj in outputs.items() if obj is not None}
    return n, d_org, d_dir, d_col, d_pix, d_smp, ptrs, bounce


def check_scene_set(flat, who):
    """The _into calls work on the scene last set."""
    if flat is None:
        raise RuntimeError(f"{who} needs a scene: call set_scene first")
