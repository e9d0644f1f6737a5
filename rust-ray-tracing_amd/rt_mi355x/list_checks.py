"""Argument checks of the ray lists (GpuRenderer.path_step_list_into, compact_list_into): everything that runs before
any GPU call and needs no library.  The rays, the counter, the colour and the step's outputs are step_checks.py's
check_path_step_into, reused and not copied; what is added here is the lists (uint32, contiguous, one entry per ray),
the counts (one uint32 word), the pairing and ping-pong rules of include/rt_mi355x.h, and the keep mask.
"""
import numpy as np

from .checks import LIVE_PATH, _device_array, _device_output, _live_path
from .step_checks import check_path_step_into

LIST_REFUSAL = "ray lists step on the live path: mode 'vectorized2' only (root2 is allowed)"


def _same_memory(a, b):
    return a is not None and b is not None and a == b


def check_lists(device, n, list_in, count_in, list_out, count_out, need_out=False):
    """The four list arguments of a call over n rays: list_in / list_out device arrays (n,) uint32 or None, count_in /
    count_out device arrays (1,) uint32 or None; the outputs writable, given together, and not the inputs.  need_out:
    a compaction, which is nothing without an output list.  Returns the four pointers (None where not given)."""
    if (list_out is None) != (count_out is None):
        raise ValueError("list_out and count_out must be given together (or neither: no output list)")
    if need_out and list_out is None:
        raise ValueError("a compaction needs an output list: list_out and count_out")
    d_li = None if list_in is None else _device_array(list_in, "list_in", np.uint32, (n,), device)
    d_ci = None if count_in is None else _device_array(count_in, "count_in", np.uint32, (1,), device)
    d_lo = None if list_out is None else _device_output(list_out, "list_out", np.uint32, (n,), device)
    d_co = None if count_out is None else _device_output(count_out, "count_out", np.uint32, (1,), device)
    if _same_memory(d_li, d_lo):
        raise ValueError("list_out is list_in: ping-pong two lists")
    if _same_memory(d_ci, d_co):
        raise ValueError("count_out is count_in: ping-pong two counts")
    return d_li, d_ci, d_lo, d_co


def check_path_step_list_into(flags, device, origins, directions, pixel, sample, colour, outputs, bounce, list_in,
                              count_in, list_out, count_out):
    """GpuRenderer.path_step_list_into's arguments checked before any GPU call: check_path_step_into's, then the
    lists.  Returns (n, d_origins, d_directions, d_colour | None, d_pixel, d_sample, {name: pointer}, bounce,
    (d_list_in, d_count_in, d_list_out, d_count_out))."""
    _live_path(flags, LIVE_PATH, LIST_REFUSAL)
    step = check_path_step_into(flags, device, origins, directions, pixel, sample, colour, outputs, bounce)
    return step + (check_lists(device, step[0], list_in, count_in, list_out, count_out),)


def check_compact_list_into(device, keep, list_out, count_out, list_in, count_in):
    """GpuRenderer.compact_list_into's arguments checked before any GPU call: keep a device array (n,) uint8 by ray id
    (n: its length, the capacity of the lists), then the lists.  Returns (n, d_keep, (d_list_in, d_count_in,
    d_list_out, d_count_out))."""
    cai = getattr(keep, "__cuda_array_interface__", None)
    if not isinstance(cai, dict) or len(cai["shape"]) != 1:
        raise TypeError("keep must be a device array of shape (n,), one uint8 per ray id")
    n = int(cai["shape"][0])
    if n > 0x7FFFFFFF:
        raise ValueError("more than 0x7FFFFFFF rays in one list")
    d_keep = _device_array(keep, "keep", np.uint8, (n,), device)
    return n, d_keep, check_lists(device, n, list_in, count_in, list_out, count_out, need_out=True)
