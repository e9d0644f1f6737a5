#!/usr/bin/env python3
"""What a fused path step costs on one GPU beside the pair of calls it replaces, same process and context: config C's
scene and frame (1920 x 1080), in fp32 and fp64, on three ray sets:

  bounce 0: the 2 073 600 pixel-centre primary rays (origins per ray: the camera centre in every row);
  bounce 1: the rays they scatter into (the scattered ones, compacted, their pixel and sample kept);
  bounce 2: the rays those scatter into.

(a) rt_path_step_async with d_status: closest hit and scatter in one kernel, the ray in registers between them;
(b) rt_query_hits_async with d_t and d_index, then rt_scatter_async in place on the same arrays: two kernels, the hit
    through memory.

The rays and the colour are uploaded again before every launch (a step updates them in place; uploads are outside the
timed span), a warm-up of each side, then the sides alternating; the median of REPS kernel_ms (rt_context_collect, HIP
events from the first to the last kernel of the side).  The tool asserts that (a) and (b) leave identical arrays.  The
claim it checks: (a) is not slower than (b) on any row, i.e. median(a) <= median(b) (1 + s) with s the larger of the
two sides' (max - min) / median over the reps.

Also recorded, without a condition: integrators.path_trace over LOOP_SPP samples per pixel (the pixel-centre ray of each
pixel, LOOP_SPP times with its own sample id) for 50 bounces, its kernel time summed over the steps, beside
rt_render_async in mode "vectorized" at the same spp and bounces: what driving the loop from the host costs.

The evidence for DESIGN.md §4 "Path steps" (profiles/path_step.txt).

    python tools/step_ab.py [--reps 7] [--loop-spp 16] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import rt_mi355x as rt  # noqa: E402
from rt_mi355x import abi, integrators  # noqa: E402
from query_ab import Device, pixel_centre_rays  # noqa: E402

SEED = 0x5EED0001
BOUNCES = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-spp", type=int, default=16)
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
    say(f"{lib.rt_version().decode()}: config C, {W} x {H}, {flat.n_spheres} spheres, medians of {args.reps}")
    ok = True
    for prec in ("f32", "f64"):
        dtype = np.float32 if prec == "f32" else np.float64
        flags = abi.RT_FLAG_F32 if prec == "f32" else 0
        r = rt.GpuRenderer(precision=prec, lib=lib, seed=SEED)
        r.set_scene(flat)
        dev = Device(lib, r.ctx)
        try:
            d = np.ascontiguousarray(pixel_centre_rays(cam, dtype).reshape(-1, 3))
            o = np.ascontiguousarray(np.broadcast_to(np.array(list(cam.center)).astype(dtype), d.shape))
            pix = np.arange(d.shape[0], dtype=np.uint32)
            smp = np.zeros(d.shape[0], dtype=np.uint32)
            col = np.ones(d.shape, dtype)
            for bounce in range(3):
                n = d.shape[0]
                d_o, d_d, d_c = dev.alloc(o.nbytes), dev.alloc(d.nbytes), dev.alloc(col.nbytes)
                d_pix, d_smp = dev.upload(pix), dev.upload(smp)
                d_st, d_idx, d_t = dev.alloc(n), dev.alloc(4 * n), dev.alloc(n * dtype().itemsize)

                def upload():
                    for ptr, a in ((d_o, o), (d_d, d), (d_c, col)):
                        abi.check(lib, lib.rt_memcpy_h2d(r.ctx, ptr, a.ctypes.data, a.nbytes))

                def side_a():
                    abi.check(lib, lib.rt_path_step_async(r.ctx, n, d_o, d_d, d_c, d_pix, d_smp, bounce, SEED, flags,
                                                          d_st, None, None, None, None, None))

                def side_b():
                    abi.check(lib, lib.rt_query_hits_async(r.ctx, n, d_o, None, d_d, flags, d_t, d_idx, None, None, None, None))
                    abi.check(lib, lib.rt_scatter_async(r.ctx, n, d_o, None, d_d, d_idx, d_t, d_pix, d_smp, bounce, SEED,
                                                        flags, d_c, d_o, d_d, None))

                res, after = {"a": [], "b": []}, {}
                for rep in range(args.reps + 1):
                    for side, fn in (("a", side_a), ("b", side_b)):
                        upload()
                        fn()
                        st = abi.RtStats()
                        abi.check(lib, lib.rt_context_collect(r.ctx, None, ctypes.byref(st)))
                        if rep:
                            res[side].append(st)
                        if rep == args.reps:
                            after[side] = [dev.download(p, a.shape, a.dtype) for p, a in ((d_o, o), (d_d, d), (d_c, col))]
                what = {"a": "rt_path_step_async", "b": "rt_query_hits_async + rt_scatter_async"}
                med, spread = {}, {}
                for side in "ab":
                    ms = [st.kernel_ms for st in res[side]]
                    med[side] = statistics.median(ms)
                    spread[side] = (max(ms) - min(ms)) / med[side]
                    st = res[side][-1]
                    say(f"{prec} bounce {bounce} ({side}) {what[side]:<40} kernel {med[side]:8.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  "
                        f"{n / med[side] / 1e3:9.1f} Mrays/s  last kernel {abi.kernel_name(st.kernel_id)}  box {st.box_groups} "
                        f"filter {st.filter_groups} exact {st.exact_tests}")
                s = max(spread.values())
                holds = med["a"] <= med["b"] * (1.0 + s)
                say(f"{prec} bounce {bounce} {n} rays  a/b {med['a'] / med['b']:.3f}   s {s:.3f}   (a) <= (b) (1 + s): {holds}")
                same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(after["a"], after["b"]))
                status = dev.download(d_st, (n,), np.uint8)
                say(f"{prec} bounce {bounce} (a) and (b) leave identical rays and colours: {same}   "
                    f"({int((status == 1).sum())} scattered, {int((status == 0).sum())} missed, {int((status == 255).sum())} invalid)")
                assert same, f"{prec} bounce {bounce}: the fused call and the pair differ"
                ok = ok and holds
                keep = status == abi.RT_STEP_SCATTERED   # the next set: the rays these scatter into
                o, d, col = (np.ascontiguousarray(a[keep]) for a in after["a"])
                pix, smp = pix[keep], smp[keep]
                dev.free()
            # the loop driven from the host beside the render that is the same computation
            spp = args.loop_spp
            d0 = np.repeat(pixel_centre_rays(cam, dtype).reshape(-1, 3), spp, axis=0)
            o0 = np.broadcast_to(np.array(list(cam.center)).astype(dtype), d0.shape)
            stats = {}
            integrators.path_trace(r, o0, d0, np.repeat(np.arange(W * H, dtype=np.uint32), spp),
                                   np.tile(np.arange(spp, dtype=np.uint32), W * H), BOUNCES, flat, seed=SEED, stats=stats)
            v = rt.GpuRenderer(precision=prec, mode="vectorized", lib=lib, seed=SEED)
            try:
                v.render_flat(BOUNCES, spp, flat, cam)   # warm-up
                _, _, st, _ = v.render_flat(BOUNCES, spp, flat, cam)
            finally:
                v.close()
            say(f"{prec} loop   integrators.path_trace, {BOUNCES} bounces x {spp} spp: {stats['steps']} steps, kernel "
                f"{stats['kernel_ms']:.2f} ms summed, {stats['ray_segments']} ray segments, {stats['invalid']} invalid lanes;  "
                f"rt_render_async (vectorized): kernel {st.kernel_ms:.2f} ms, {st.ray_segments} ray segments;  "
                f"loop / render {stats['kernel_ms'] / st.kernel_ms:.2f}")
        finally:
            dev.free()
            r.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
