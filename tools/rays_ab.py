#!/usr/bin/env python3
"""What rendering caller-supplied rays costs on one GPU (rt_render_rays_async), same process and context: config C's
frame (1920 x 1080), scene and bounce count, in fp32 and fp64.

(p16, p512)  a 360 degree panorama from the camera's centre (rt.projections.equirect, grid = 1: one ray per pixel,
             per-ray origins) at spp 16 and at spp 512;
(r16, r512)  beside them rt_render_async with the perspective camera at the same pixel count and spp;
(c16, c512)  the perspective camera's own pixel-centre rays (one per pixel, no jitter) through rt_render_rays_async:
             the render's frame through the ray path, for a like-for-like cost.

(p) and (r) do not trace the same rays (a panorama sees the whole sphere of directions, most of it sky and ground), so
their ratio is the cost of a frame through each entry point, not of one path: ray_segments per sample is printed with
it.  (c) and (r) see the same spheres from the same pixels.
The ray path sends bounce 0 through the general sweep, reads its rays from memory and finishes no sky pixel at claim
time; the render runs camera batches and direct sky pixels.

A warm-up of each side, then the sides alternating; the median of REPS kernel_ms (rt_context_collect, HIP events; the
rays are on the device before, the image stays there).  No threshold: the numbers are what comes out.

The evidence for DESIGN.md §4 "Caller-supplied primary rays" (profiles/rays.txt).

    python tools/rays_ab.py [--reps 7] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import rt_mi355x as rt  # noqa: E402
from rt_mi355x import abi  # noqa: E402
from query_ab import Device, pixel_centre_rays  # noqa: E402

SEED = 0x5EED0001


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
    W, H, _, _, depth = rt.scenes.CONFIGS["C"]
    flat = rt.scenes.config_scene("C").flatten()
    cam = rt.camera_new_py(W, H, **rt.MAIN_CAMERA)
    n = W * H
    say(f"{lib.rt_version().decode()}: config C, {W} x {H} = {n} pixels, {flat.n_spheres} spheres, {depth} bounces, "
        f"medians of {args.reps}")
    for prec in ("f32", "f64"):
        flags = abi.RT_FLAG_F32 if prec == "f32" else 0
        r = rt.GpuRenderer(precision=prec, lib=lib)
        dev = Device(lib, r.ctx)
        try:
            r.set_scene(flat)
            o, d = rt.projections.equirect(W, H, rt.MAIN_CAMERA["center"], rt.MAIN_CAMERA["look_at"], rt.MAIN_CAMERA["up"],
                                           grid=1, precision=prec, lib=lib)
            d_org, d_dir, d_rgb = dev.upload(o), dev.upload(d), dev.alloc(n * 3)
            c_dir = dev.upload(pixel_centre_rays(cam, d.dtype))   # their origin: the panorama's, the camera centre

            def rays(spp, dirs=None):
                abi.check(lib, lib.rt_render_rays_async(r.ctx, n, spp, 1, d_org, None, dirs or d_dir, depth, SEED, 0, flags,
                                                        d_rgb, None, None))
                st = abi.RtStats()
                abi.check(lib, lib.rt_context_collect(r.ctx, None, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
                assert st.samples == n * spp and abi.RT_KERNEL_RAYS(st.kernel_id)
                return st

            def render(spp):
                abi.check(lib, lib.rt_render_async(r.ctx, ctypes.byref(cam), depth, spp, SEED, flags, None, d_rgb, None, None))
                st = abi.RtStats()
                abi.check(lib, lib.rt_context_collect(r.ctx, None, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
                assert st.samples == n * spp and not abi.RT_KERNEL_RAYS(st.kernel_id)
                return st

            sides = [("p16", lambda: rays(16)), ("r16", lambda: render(16)), ("c16", lambda: rays(16, c_dir)),
                     ("p512", lambda: rays(512)), ("r512", lambda: render(512)), ("c512", lambda: rays(512, c_dir))]
            what = {"p16": "panorama rays, 16 spp", "r16": "rt_render_async, 16 spp", "c16": "camera's rays, 16 spp",
                    "p512": "panorama rays, 512 spp", "r512": "rt_render_async, 512 spp", "c512": "camera's rays, 512 spp"}
            res = {k: [] for k, _ in sides}
            for rep in range(args.reps + 1):
                for name, fn in sides:
                    st = fn()
                    if rep:
                        res[name].append(st)
            med = {}
            for name, _ in sides:
                ms = [st.kernel_ms for st in res[name]]
                med[name] = statistics.median(ms)
                st = res[name][-1]
                say(f"{prec} ({name:<4}) {what[name]:<26} kernel {med[name]:9.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  "
                    f"{st.samples / med[name] / 1e6:7.2f} Gsamples/s  {st.ray_segments / st.samples:5.2f} segments/sample  "
                    f"{st.ray_segments / med[name] / 1e6:7.2f} Gsegments/s  direct sky {st.direct_sky_samples / st.samples:.3f}  "
                    f"{abi.kernel_name(st.kernel_id)}")
            for spp in (16, 512):
                p, q = res[f"p{spp}"][-1], res[f"r{spp}"][-1]
                say(f"{prec} spp {spp}: panorama / render, time per frame {med[f'p{spp}'] / med[f'r{spp}']:.3f}, "
                    f"time per ray segment {(med[f'p{spp}'] / p.ray_segments) / (med[f'r{spp}'] / q.ray_segments):.3f};  "
                    f"camera's rays / render, time per frame {med[f'c{spp}'] / med[f'r{spp}']:.3f}")
        finally:
            dev.free()
            r.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
