#!/usr/bin/env python3
"""What a ray query costs on one GPU (rt_query_hits_async), same process and context: config C's frame (1920 x 1080,
one primary ray through every pixel's centre) over config C's scene, in fp32 and fp64, RT_FLAG_ROOT2 off.

(a) the rays in pixel order through the general path (per-ray origins, all equal to the camera centre);
(b) the same rays shuffled (a fixed permutation), general path: what incoherent batches cost;
(c) the same rays in pixel order through the shared-origin path (the camera sweep over the centre's tables);
(g) beside them rt_render_guides_async at spp = 1: the same first hits, found through the per-pixel candidate lists.

A warm-up of each side, then the sides alternating; the median of REPS kernel_ms (rt_context_collect, HIP events;
the rays are on the device before, the results stay there).  No threshold: the numbers are what comes out.  The one
condition is that (a), (b) unshuffled and (c) return identical arrays, all five outputs, bit for bit.

The evidence for DESIGN.md §4 "Ray queries" (profiles/query.txt).

    python tools/query_ab.py [--reps 7] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
import rt_mi355x as rt  # noqa: E402
from rt_mi355x import abi  # noqa: E402
from rt_mi355x.renderer import QUERY_NAMES, QUERY_OUTPUTS  # noqa: E402


def pixel_centre_rays(cam, dtype):
    """Camera::get_ray with both jitter draws at 0.5 and no defocus offset, for every pixel in pixel order, in dtype."""
    t = np.dtype(dtype).type
    W, H = cam.image_width, cam.image_height
    fx = ((np.arange(W, dtype=dtype) + t(0.5)) / t(W))[None, :, None]
    fy = ((np.arange(H, dtype=dtype) + t(0.5)) / t(H))[:, None, None]
    vu, vv, ulc, cen = (np.array(list(v), dtype=dtype) for v in (cam.vu, cam.vv, cam.ulc, cam.center))
    v = ((ulc + (vu * fx + vv * fy)) - cen).reshape(-1, 3)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return np.ascontiguousarray(v / ln[:, None], dtype=dtype)


class Device:
    """Device buffers of one context, freed together."""

    def __init__(self, lib, ctx):
        self.lib, self.ctx, self.ptrs = lib, ctx, []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        abi.check(self.lib, self.lib.rt_device_alloc(self.ctx, nbytes, ctypes.byref(p)))
        self.ptrs.append(p)
        return p

    def upload(self, a):
        p = self.alloc(a.nbytes)
        abi.check(self.lib, self.lib.rt_memcpy_h2d(self.ctx, p, a.ctypes.data, a.nbytes))
        return p

    def download(self, p, shape, dtype):
        a = np.empty(shape, dtype)
        abi.check(self.lib, self.lib.rt_memcpy_d2h(self.ctx, a.ctypes.data, p, a.nbytes))
        return a

    def free(self):
        for p in self.ptrs:
            self.lib.rt_device_free(self.ctx, p)
        self.ptrs = []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = rt.load_library()
    W, H = rt.scenes.CONFIGS["C"][:2]
    flat = rt.scenes.config_scene("C").flatten()
    cam = rt.camera_new_py(W, H, **rt.MAIN_CAMERA)
    n = W * H
    say(f"{lib.rt_version().decode()}: config C, {W} x {H} = {n} rays, {flat.n_spheres} spheres, medians of {args.reps}")
    ok = True
    for prec in ("f32", "f64"):
        dtype = np.float32 if prec == "f32" else np.float64
        flags = abi.RT_FLAG_F32 if prec == "f32" else 0
        r = rt.GpuRenderer(precision=prec, lib=lib)
        dev = Device(lib, r.ctx)
        try:
            r.set_scene(flat)
            d = pixel_centre_rays(cam, dtype)
            o = np.ascontiguousarray(np.broadcast_to(np.array(list(cam.center), dtype=dtype), d.shape))
            perm = np.random.default_rng(0xC).permutation(n)
            d_dir, d_org = dev.upload(d), dev.upload(o)
            d_dir_s = dev.upload(np.ascontiguousarray(d[perm]))
            centre = (ctypes.c_double * 3)(*cam.center)
            shapes = {k: ((n, 3) if QUERY_OUTPUTS[k][0] == 3 else (n,), QUERY_OUTPUTS[k][1] or dtype) for k in QUERY_NAMES}
            outs = {side: {k: dev.alloc(int(np.prod(s)) * np.dtype(t).itemsize) for k, (s, t) in shapes.items()}
                    for side in "abc"}

            def query(side):
                shared = side == "c"
                abi.check(lib, lib.rt_query_hits_async(r.ctx, n, None if shared else d_org, centre if shared else None,
                                                       d_dir_s if side == "b" else d_dir, flags,
                                                       *[outs[side][k] for k in QUERY_NAMES], None))
                st = abi.RtStats()
                abi.check(lib, lib.rt_context_collect(r.ctx, None, ctypes.byref(st)))
                assert st.samples == n and abi.RT_KERNEL_QUERY(st.kernel_id)
                return st

            def guides():
                _, st, _ = r.guides_flat(1, flat, cam, want=("depth",))
                return st

            sides = [("a", lambda: query("a")), ("b", lambda: query("b")), ("c", lambda: query("c")), ("g", guides)]
            res = {k: [] for k, _ in sides}
            for rep in range(args.reps + 1):
                for name, fn in sides:
                    st = fn()
                    if rep:
                        res[name].append(st)
            what = {"a": "general path, pixel order", "b": "general path, shuffled", "c": "shared origin, pixel order",
                    "g": "rt_render_guides_async, 1 spp"}
            med = {}
            for name, _ in sides:
                ms = [st.kernel_ms for st in res[name]]
                med[name] = statistics.median(ms)
                st = res[name][-1]
                say(f"{prec} ({name}) {what[name]:<30} kernel {med[name]:8.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  "
                    f"{n / med[name] / 1e3:9.1f} Mrays/s  {abi.kernel_name(st.kernel_id)}  lane_slots {st.lane_slots}  "
                    f"box {st.box_groups} filter {st.filter_groups} exact {st.exact_tests} cone {st.cone_tests} "
                    f"camera_exact {st.camera_exact_tests}")
            say(f"{prec} b/a {med['b'] / med['a']:.3f}   c/a {med['c'] / med['a']:.3f}   c/g {med['c'] / med['g']:.3f}")
            same_prec = True
            got = {side: {k: dev.download(outs[side][k], *shapes[k]) for k in QUERY_NAMES} for side in "abc"}
            for k in QUERY_NAMES:
                unshuffled = np.empty_like(got["b"][k])
                unshuffled[perm] = got["b"][k]
                for side, a in (("b", unshuffled), ("c", got["c"][k])):
                    same = a.tobytes() == got["a"][k].tobytes()
                    same_prec = same_prec and same
                    if not same:
                        say(f"{prec} MISMATCH: {k} of ({side}) differs from (a) in {int((a != got['a'][k]).sum())} elements")
            hits = int((got["a"]["index"] >= 0).sum())
            ok = ok and same_prec
            say(f"{prec} (a), (b) unshuffled and (c) identical in all five outputs: {same_prec}   ({hits} of {n} rays hit)")
        finally:
            dev.free()
            r.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
