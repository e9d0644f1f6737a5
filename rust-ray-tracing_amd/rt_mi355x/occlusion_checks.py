"""Argument checks of the occlusion queries (GpuRenderer.occluded, occluded_into): everything that runs before any
GPU call and needs no library.  The ray checks are checks.py's, the ones a ray query takes (check_query,
check_query_into), reused and not copied; what is added here is t_max, the output array and the scene.
"""
import numpy as np

from .checks import (LIVE_PATH, QUERY_RAYS, _device_array, _device_output, _device_rays, _host_rays, _live_path,
                     _query_count)


def _numbers(t):
    if t.dtype.kind not in "fiu":
        raise ValueError(f"t_max must be a number or an array of numbers, not dtype {t.dtype}")


def _scalar_t_max(t_max):
    """One bound for every ray: a number that is not NaN (the library refuses NaN).  Returns a float."""
    t = np.asarray(t_max)
    _numbers(t)
    t = float(t)
    if t != t:
        raise ValueError("t_max is NaN (a per-ray array may hold NaN: such a ray is invalid)")
    return t


def check_occluded(flags, origins, directions, t_max=np.inf):
    """GpuRenderer.occluded's arguments checked before any GPU call: check_query's ray checks, and t_max a number
    (not NaN) or an (n,) array of numbers.  Returns (origins, directions, shared, t_max): the arrays contiguous in the
    renderer's precision, a shared origin kept in float64, t_max a float or an (n,) array in that precision."""
    dtype = _live_path(flags, LIVE_PATH, QUERY_RAYS.refusal)
    o, d, shared = _host_rays(dtype, origins, directions, QUERY_RAYS, _query_count)
    t = np.asarray(t_max)
    if t.ndim == 0:
        return o, d, shared, _scalar_t_max(t)
    _numbers(t)
    if t.shape != (d.shape[0],):
        raise ValueError(f"t_max must be a number or have shape ({d.shape[0]},), one bound per ray, not {t.shape}")
    with np.errstate(over="ignore"):   # a float64 bound above the largest float32 is +inf: unbounded
        t = np.ascontiguousarray(t, dtype=dtype)
    return o, d, shared, t


def check_occluded_into(flags, device, origins, directions, occluded, t_max=np.inf):
    """GpuRenderer.occluded_into's arguments checked before any GPU call: check_query_into's ray checks, occluded a
    writable device array (n,) of uint8, t_max a number (not NaN) or a device array (n,) of the renderer's precision.
    Returns (n, d_origins | None, origin | None, d_directions, d_t_max | None, t_max: float, d_occluded)."""
    dtype = _live_path(flags, LIVE_PATH, QUERY_RAYS.refusal)
    n, _, d_org, origin, d_dir = _device_rays(dtype, device, origins, directions, QUERY_RAYS, _query_count)
    d_occ = _device_output(occluded, "occluded", np.uint8, (n,), device)
    if hasattr(t_max, "__cuda_array_interface__"):
        return n, d_org, origin, d_dir, _device_array(t_max, "t_max", dtype, (n,), device), 0.0, d_occ
    if np.ndim(t_max) != 0:
        raise TypeError("t_max must be a number or a device array exposing __cuda_array_interface__")
    return n, d_org, origin, d_dir, None, _scalar_t_max(t_max), d_occ


def check_scene_set(flat):
    """occluded_into works on the scene last set."""
    if flat is None:
        raise RuntimeError("occluded_into needs a scene: call set_scene first")
