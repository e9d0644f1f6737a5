#!/usr/bin/env python3
"""What an occlusion query costs on one GPU beside what a caller did before it existed, same process and context:
config C's scene and frame (1920 x 1080), in fp32 and fp64.  The rays start at the `point` of every pixel-centre
first hit (rt_query_hits_async, RT_FLAG_ROOT2, shared origin); pixels that hit nothing send no ray.

Workload 1, shadow rays: d = L - p towards a fixed point light L, t_max = 1 (the open segment up to the light).
Workload 2, AO rays:     4 seeded unit directions per hit point in the normal's hemisphere, t_max = 2.0, pixel order.

(a) rt_query_occluded_async: one byte per ray, the any-hit sweep bounded by t_max;
(b) rt_query_hits_async with only d_t on the same rays, the closest hit over the whole hierarchy; the caller then
    compares t < t_max on the host (not timed).

A warm-up of each side, then the sides alternating; the median of REPS kernel_ms (rt_context_collect, HIP events; the
rays are on the device before, the results stay there), and each side's work counters.  The tool asserts that (a) and
(b) agree on every ray.  The claim it checks: (a) is not slower than (b), i.e. median(a) <= median(b) (1 + s) with s
the larger of the two sides' (max - min) / median over the reps (these are launches of a fraction of a millisecond).

The evidence for DESIGN.md §4 "Occlusion queries" (profiles/occlusion.txt).

    python tools/occlusion_ab.py [--reps 7] [--out FILE]
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
from rt_mi355x import abi  # noqa: E402
from query_ab import Device, pixel_centre_rays  # noqa: E402

LIGHT = (-6.0, 18.0, 9.0)
AO_RAYS, AO_T_MAX = 4, 2.0


def hemisphere(normal, rng, dtype):
    """AO_RAYS unit directions per normal, uniform on the sphere and flipped into the normal's hemisphere: [n, AO_RAYS, 3]."""
    v = rng.standard_normal((normal.shape[0], AO_RAYS, 3))
    v /= np.sqrt((v * v).sum(-1, keepdims=True))
    v *= np.where((v * normal[:, None, :].astype(np.float64)).sum(-1, keepdims=True) < 0, -1.0, 1.0)
    return v.astype(dtype)


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
    say(f"{lib.rt_version().decode()}: config C, {W} x {H}, {flat.n_spheres} spheres, light {LIGHT}, medians of {args.reps}")
    ok = True
    for prec in ("f32", "f64"):
        dtype = np.float32 if prec == "f32" else np.float64
        flags = (abi.RT_FLAG_F32 if prec == "f32" else 0) | abi.RT_FLAG_ROOT2
        r = rt.GpuRenderer(precision=prec, lib=lib)
        dev = Device(lib, r.ctx)
        try:
            first = r.query(np.array(list(cam.center)), pixel_centre_rays(cam, dtype), flat, root2=True,
                            want=("index", "point", "normal"))
            hit = first["index"] >= 0
            p, nrm = first["point"][hit], first["normal"][hit]
            light = np.array(LIGHT, dtype=dtype)
            work = {"shadow": (p, np.ascontiguousarray(light[None, :] - p), 1.0),
                    "ao": (np.ascontiguousarray(np.repeat(p, AO_RAYS, 0)),
                           np.ascontiguousarray(hemisphere(nrm, np.random.default_rng(0xA0), dtype).reshape(-1, 3)), AO_T_MAX)}
            for name, (o, d, t_max) in work.items():
                n = d.shape[0]
                d_org, d_dir = dev.upload(np.ascontiguousarray(o)), dev.upload(d)
                d_occ, d_t = dev.alloc(n), dev.alloc(n * dtype().itemsize)

                def side_a():
                    abi.check(lib, lib.rt_query_occluded_async(r.ctx, n, d_org, None, d_dir, None, t_max, flags, d_occ, None))

                def side_b():
                    abi.check(lib, lib.rt_query_hits_async(r.ctx, n, d_org, None, d_dir, flags, d_t, None, None, None, None, None))

                res = {"a": [], "b": []}
                for rep in range(args.reps + 1):
                    for side, fn in (("a", side_a), ("b", side_b)):
                        fn()
                        st = abi.RtStats()
                        abi.check(lib, lib.rt_context_collect(r.ctx, None, ctypes.byref(st)))
                        if rep:
                            res[side].append(st)
                what = {"a": "rt_query_occluded_async", "b": "rt_query_hits_async, d_t only"}
                med, spread = {}, {}
                for side in "ab":
                    ms = [st.kernel_ms for st in res[side]]
                    med[side] = statistics.median(ms)
                    spread[side] = (max(ms) - min(ms)) / med[side]
                    st = res[side][-1]
                    say(f"{prec} {name:<6} ({side}) {what[side]:<30} kernel {med[side]:8.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  "
                        f"{n / med[side] / 1e3:9.1f} Mrays/s  {abi.kernel_name(st.kernel_id)}  samples {st.samples} "
                        f"lane_slots {st.lane_slots}  box {st.box_groups} filter {st.filter_groups} exact {st.exact_tests}")
                s = max(spread.values())
                holds = med["a"] <= med["b"] * (1.0 + s)
                say(f"{prec} {name:<6} a/b {med['a'] / med['b']:.3f}   s {s:.3f}   (a) <= (b) (1 + s): {holds}")
                occ = dev.download(d_occ, (n,), np.uint8)
                t = dev.download(d_t, (n,), dtype)
                with np.errstate(invalid="ignore"):
                    host = np.where(np.isnan(t), abi.RT_OCCLUDED_INVALID, t < dtype(t_max)).astype(np.uint8)
                same = bool((occ == host).all())
                say(f"{prec} {name:<6} {n} rays, (a) and (b) agree on every ray: {same}   "
                    f"({int((occ == 1).sum())} occluded, {int((occ == 255).sum())} invalid)")
                assert same, f"{prec} {name}: {(occ != host).sum()} rays differ"
                ok = ok and holds
        finally:
            dev.free()
            r.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
