"""Primary rays of the camera models the reference lacks, through rt_camera_rays (include/rt_mi355x.h): host arrays
for GpuRenderer.render_rays (full paths) or GpuRenderer.query (first hits).  No GPU is needed to make them.

Each function returns (origins, directions) shaped (H * W, grid * grid, 3) in float64, or float32 for
precision="f32": pixels row-major from the top left, and within a pixel ray j * grid + i through the sub-pixel
position ((i + 0.5) / grid, (j + 0.5) / grid).  The frame is the perspective camera's: look_from, look_at, up.
"""
import ctypes

import numpy as np

from . import abi

MODELS = {"ortho": abi.RT_PROJ_ORTHOGRAPHIC, "equirect": abi.RT_PROJ_EQUIRECT, "fisheye": abi.RT_PROJ_FISHEYE}


def camera_rays(model, width, height, look_from, look_at, up=(0.0, 1.0, 0.0), grid=1, precision="f64", angle_deg=180.0,
                extent=1.0, lib=None):
    """rt_camera_rays for model "ortho", "equirect" or "fisheye" (or an abi.RT_PROJ_* value)."""
    if precision not in ("f64", "f32"):
        raise ValueError(f"unknown precision {precision!r}")
    if isinstance(model, str):
        if model not in MODELS:
            raise ValueError(f"unknown projection {model!r} (one of {sorted(MODELS)})")
        model = MODELS[model]
    width, height, grid = int(width), int(height), int(grid)
    if width <= 0 or height <= 0 or grid <= 0:
        raise ValueError("width, height and grid must be positive")
    lib = lib or abi.load_library()
    proj = abi.RtProjection(model, width, height, (abi.f64 * 3)(*look_from), (abi.f64 * 3)(*look_at), (abi.f64 * 3)(*up),
                            float(angle_deg), float(extent))
    dtype = np.float32 if precision == "f32" else np.float64
    shape = (width * height, grid * grid, 3)
    origins, directions = np.empty(shape, dtype), np.empty(shape, dtype)
    abi.check(lib, lib.rt_camera_rays(ctypes.byref(proj), grid, abi.RT_FLAG_F32 if precision == "f32" else 0,
                                      origins.ctypes.data, directions.ctypes.data))
    return origins, directions


def orthographic(width, height, look_from, look_at, up=(0.0, 1.0, 0.0), extent=1.0, grid=1, precision="f64", lib=None):
    """Parallel rays along the view axis; the origins lie on a plane through look_from, `extent` world units high and
    extent * width / height wide."""
    return camera_rays("ortho", width, height, look_from, look_at, up, grid, precision, extent=extent, lib=lib)


def equirect(width, height, look_from, look_at, up=(0.0, 1.0, 0.0), grid=1, precision="f64", lib=None):
    """A 360 x 180 degree panorama from look_from: longitude over the columns (the view axis in the middle column),
    latitude over the rows (up at the top)."""
    return camera_rays("equirect", width, height, look_from, look_at, up, grid, precision, lib=lib)


def fisheye(width, height, look_from, look_at, up=(0.0, 1.0, 0.0), angle_deg=180.0, grid=1, precision="f64", lib=None):
    """An equidistant fisheye of angle_deg degrees across the shorter side.  Rays outside the image circle have the
    direction 0, 0, 0: invalid rays, so their pixels render black."""
    return camera_rays("fisheye", width, height, look_from, look_at, up, grid, precision, angle_deg=angle_deg, lib=lib)
