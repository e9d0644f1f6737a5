#!/usr/bin/env python3
"""What ray lists buy a caller-driven path tracer on one GPU, same process and context: config C's scene and frame
(1920 x 1080), in fp32 and fp64.

The loop (the claim): integrators.path_trace over LOOP_SPP samples per pixel (the pixel-centre ray of each pixel,
LOOP_SPP times with its own sample id) for 50 bounces,
  (a) compact=True: rt_path_step_list_async over the live rays, the next list left on the device, 4 bytes to the host
      per step;
  (b) compact=False: rt_path_step_async over every slot, the status bytes and the directions to the host per step.
Kernel time is the steps' kernel_ms summed (HIP events, rt_context_collect; (a)'s spans include the compaction
kernels), wall time the whole call.  One warm-up of each side, then the sides alternating; medians of REPS.  The tool
asserts that (a) and (b) return identical ray_segments, samples, steps and invalid, and identical radiance except at the
rays whose final status is invalid (0 under (a), the plain loop's sky term under (b); stats["invalid"] counts them).  The claim it checks:
median(a) <= median(b) (1 + s) in kernel time, s the larger of the two sides' (max - min) / median.  Beside them:
rt_render_async in mode "vectorized" at the same spp and bounces, re-measured here.

Per step (recorded, no condition): bounce 0, 1 and 2 of the pixel-centre primary rays,
  (a) rt_path_step_list_async with an output list: the identity list at bounce 0, the surviving list after;
  (b) rt_path_step_async over all 2 073 600 slots, the retired rays' directions zeroed as path_trace leaves them.
The arrays are uploaded again before every launch (outside the timed span).  The tool asserts that both leave
identical rays and colours.  At bounce 0 (a) does strictly more work: the compaction is what the later steps' saving
costs.

The evidence for DESIGN.md §4 "Ray lists" (profiles/ray_lists.txt).

    python tools/list_ab.py [--reps 7] [--loop-spp 16] [--prec f32,f64] [--skip-loop] [--skip-steps] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import rt_mi355x as rt  # noqa: E402
from rt_mi355x import abi, integrators  # noqa: E402
from query_ab import Device, pixel_centre_rays  # noqa: E402

SEED = 0x5EED0001
BOUNCES = 50


def med_spread(xs):
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m


def steps(say, lib, r, cam, flat, prec, reps):
    dtype = np.float32 if prec == "f32" else np.float64
    flags = abi.RT_FLAG_F32 if prec == "f32" else 0
    dev = Device(lib, r.ctx)
    try:
        d = np.ascontiguousarray(pixel_centre_rays(cam, dtype).reshape(-1, 3))
        n = d.shape[0]
        o = np.ascontiguousarray(np.broadcast_to(np.array(list(cam.center)).astype(dtype), d.shape))
        col = np.ones(d.shape, dtype)
        d_pix, d_smp = dev.upload(np.arange(n, dtype=np.uint32)), dev.upload(np.zeros(n, dtype=np.uint32))
        d_o, d_d, d_c, d_st = dev.alloc(o.nbytes), dev.alloc(d.nbytes), dev.alloc(col.nbytes), dev.alloc(n)
        d_li, d_ci, d_lo, d_co = dev.alloc(4 * n), dev.alloc(4), dev.alloc(4 * n), dev.alloc(4)
        live = np.arange(n, dtype=np.uint32)
        for bounce in range(3):
            count = np.array([live.size], np.uint32)
            first = bounce == 0

            def upload():
                for ptr, a in ((d_o, o), (d_d, d), (d_c, col), (d_li, live), (d_ci, count)):
                    abi.check(lib, lib.rt_memcpy_h2d(r.ctx, ptr, a.ctypes.data, a.nbytes))

            def side_a():
                abi.check(lib, lib.rt_path_step_list_async(r.ctx, n, None if first else d_li, None if first else d_ci, d_o,
                                                           d_d, d_c, d_pix, d_smp, bounce, SEED, flags, d_st, None, None,
                                                           None, None, d_lo, d_co, None))

            def side_b():
                abi.check(lib, lib.rt_path_step_async(r.ctx, n, d_o, d_d, d_c, d_pix, d_smp, bounce, SEED, flags, d_st,
                                                      None, None, None, None, None))

            res, after = {"a": [], "b": []}, {}
            for rep in range(reps + 1):
                for side, fn in (("a", side_a), ("b", side_b)):
                    upload()
                    fn()
                    st = abi.RtStats()
                    abi.check(lib, lib.rt_context_collect(r.ctx, None, ctypes.byref(st)))
                    if rep:
                        res[side].append(st)
                    if rep == reps:
                        after[side] = [dev.download(p, a.shape, a.dtype) for p, a in ((d_o, o), (d_d, d), (d_c, col))]
            what = {"a": "rt_path_step_list_async + output list", "b": "rt_path_step_async, all slots"}
            med = {}
            for side in "ab":
                ms = [st.kernel_ms for st in res[side]]
                med[side], _ = med_spread(ms)
                st = res[side][-1]
                say(f"{prec} bounce {bounce} ({side}) {what[side]:<40} kernel {med[side]:8.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  "
                    f"{st.samples} valid rays  lane_slots {st.lane_slots}  last kernel {abi.kernel_name(st.kernel_id)}")
            same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(after["a"], after["b"]))
            k = int(dev.download(d_co, (1,), np.uint32)[0])
            nxt = dev.download(d_lo, (n,), np.uint32)[:k].copy()
            status = dev.download(d_st, (n,), np.uint8)   # side (b)'s, the last to run: every slot
            want = live[status[live] == abi.RT_STEP_SCATTERED]
            say(f"{prec} bounce {bounce} {live.size} live of {n} slots  a/b {med['a'] / med['b']:.3f}   identical rays and "
                f"colours: {same}   next list {k} rays, as numpy has it: {np.array_equal(nxt, want)}")
            assert same and np.array_equal(nxt, want), f"{prec} bounce {bounce}: the list step and the plain step differ"
            o, d, col = after["a"]
            gone = np.ones(n, bool)
            gone[nxt] = False
            d[gone] = 0   # retired: what path_trace(compact=False) leaves for the plain step
            live = nxt
    finally:
        dev.free()


def loop(say, lib, r, cam, flat, prec, reps, spp):
    dtype = np.float32 if prec == "f32" else np.float64
    W, H = cam.image_width, cam.image_height
    d0 = np.repeat(pixel_centre_rays(cam, dtype).reshape(-1, 3), spp, axis=0)
    o0 = np.broadcast_to(np.array(list(cam.center)).astype(dtype), d0.shape)
    pix = np.repeat(np.arange(W * H, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), W * H)
    res, out = {"a": [], "b": []}, {}
    for rep in range(reps + 1):
        for side in "ab":
            stats = {}
            t0 = time.perf_counter()
            rad = integrators.path_trace(r, o0, d0, pix, smp, BOUNCES, flat, seed=SEED, stats=stats, compact=side == "a")
            stats["wall_ms"] = (time.perf_counter() - t0) * 1e3
            print(f"  {prec} loop rep {rep} ({side}): kernel {stats['kernel_ms']:.2f} ms, wall {stats['wall_ms']:.0f} ms", flush=True)
            if rep:
                res[side].append(stats)
            if rep == reps:
                out[side] = rad
            del rad
    # a ray whose final status is invalid is 0 under compact=True and keeps the plain loop's sky term under
    # compact=False: the two agree wherever no lane reports 255, so at most stats["invalid"] rays may differ
    n = out["a"].shape[0]
    rows = (out["a"].view(np.uint8).reshape(n, -1) != out["b"].view(np.uint8).reshape(n, -1)).any(axis=1)
    differ = int(rows.sum())
    same = differ <= res["a"][-1]["invalid"] and bool((out["a"][rows] == 0).all())
    keys = ("ray_segments", "samples", "steps", "invalid")
    same_stats = all(res["a"][-1][k] == res["b"][-1][k] for k in keys)
    v = rt.GpuRenderer(precision=prec, mode="vectorized", lib=lib, seed=SEED)
    try:
        v.render_flat(BOUNCES, spp, flat, cam)   # warm-up
        render = [v.render_flat(BOUNCES, spp, flat, cam)[2].kernel_ms for _ in range(reps)]
    finally:
        v.close()
    rm, _ = med_spread(render)
    what = {"a": "compact=True ", "b": "compact=False"}
    med, spread = {}, {}
    for side in "ab":
        ms = [s["kernel_ms"] for s in res[side]]
        wall = [s["wall_ms"] for s in res[side]]
        med[side], spread[side] = med_spread(ms)
        s = res[side][-1]
        say(f"{prec} loop ({side}) path_trace {what[side]} {BOUNCES} bounces x {spp} spp: {s['steps']} steps, kernel "
            f"{med[side]:8.2f} ms summed [{min(ms):.2f}..{max(ms):.2f}]  wall {statistics.median(wall):9.1f} ms  "
            f"{s['ray_segments']} ray segments, {s['invalid']} invalid;  loop / render {med[side] / rm:.2f}")
    s = max(spread.values())
    holds = med["a"] <= med["b"] * (1.0 + s)
    say(f"{prec} loop   rt_render_async (vectorized) kernel {rm:.2f} ms [{min(render):.2f}..{max(render):.2f}];  a/b "
        f"{med['a'] / med['b']:.3f}   s {s:.3f}   (a) <= (b) (1 + s): {holds};  radiance differs at {differ} rays (the invalid ones, 0 under (a)): {same}, "
        f"identical stats: {same_stats}")
    assert same and same_stats, f"{prec}: the compacted loop and the plain loop differ"
    return holds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-spp", type=int, default=16)
    ap.add_argument("--prec", default="f32,f64")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:   # as it goes: a long run leaves what it had
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    lib = rt.load_library()
    W, H = rt.scenes.CONFIGS["C"][:2]
    flat = rt.scenes.config_scene("C").flatten()
    cam = rt.camera_new_py(W, H, **rt.MAIN_CAMERA)
    say(f"{lib.rt_version().decode()}: config C, {W} x {H}, {flat.n_spheres} spheres, medians of {args.reps}")
    ok = True
    for prec in args.prec.split(","):
        r = rt.GpuRenderer(precision=prec, lib=lib, seed=SEED)
        r.set_scene(flat)
        try:
            if not args.skip_steps:
                steps(say, lib, r, cam, flat, prec, args.reps)
            if not args.skip_loop:
                ok = loop(say, lib, r, cam, flat, prec, args.reps, args.loop_spp) and ok
        finally:
            r.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
