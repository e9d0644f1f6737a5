#!/usr/bin/env python3
"""The price of a progressive session on one GPU, same process and context, by the method of tools/split_ab.py:
a warm-up of each side, then the sides alternating, the median of REPS kernel_ms (rt_context_collect, HIP events).

Sides per shape:
  (a) rt_render_async at the final spp;
  (b) a session extended to the final spp in one step, with the image;
  (c) a session on a doubling schedule from 16 spp to the final spp, the image at every step (the sum of the
      steps' kernel_ms).
Reports (b)/(a), the price of tracing through the record buffer, and (c)/(b), the price of the intermediate
images and of the smaller launches.  Every side's final image must be the same.  The record buffer's
allocation (rt_progressive_begin) is outside kernel_ms.  The evidence for DESIGN.md §4 "Progressive sessions"
(profiles/progressive.txt).

    python tools/progressive_ab.py [--reps 7] [--shapes 0,1] [--out FILE]
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

# (config scene, width, height, final spp, precision)
SHAPES = [("C", 64, 36, 4096, "f32"), ("C", 240, 135, 512, "f32"), ("C", 1920, 1080, 64, "f32"), ("C", 64, 36, 4096, "f64")]


def doubling(final):
    counts, n = [], 16
    while n < final:
        counts.append(n)
        n *= 2
    return counts + [final]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="", help="indices into SHAPES, comma separated (default: all)")
    args = ap.parse_args()
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")] if args.shapes else SHAPES
    lib = rt.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"{lib.rt_version().decode()}  reps {args.reps} (median kernel_ms; alternating a / b / c after one warm-up of each)")
    scenes = {}
    for config, w, h, spp, prec in shapes:
        flat = scenes.setdefault(config, rt.scenes.config_scene(config).flatten())
        depth = rt.scenes.CONFIGS[config][4]
        cam = rt.camera_new_py(w, h, **rt.MAIN_CAMERA)
        r = rt.GpuRenderer(precision=prec, lib=lib)
        nbytes = ctypes.c_uint64()
        abi.check(lib, lib.rt_progressive_bytes(w * h, spp, depth, r.flags, ctypes.byref(nbytes)))
        schedule = doubling(spp)

        def side_a():
            rgb, _, st, rc = r.render_flat(depth, spp, flat, cam)
            assert rc == 0
            return rgb, st.kernel_ms, st.ray_segments

        def side_session(counts):
            ms = segs = 0
            with r.begin_progressive(depth, spp, flat, cam) as s:
                for n in counts:
                    rgb, _, st, rc = s.extend(n)
                    ms += st.kernel_ms
                    segs += st.ray_segments
            assert rc == 0   # at the final count
            return rgb, ms, segs

        sides = [("a", side_a), ("b", lambda: side_session([spp])), ("c", lambda: side_session(schedule))]
        try:
            image, ms = {}, {k: [] for k, _ in sides}
            for rep in range(args.reps + 1):   # rep 0: warm-up
                for name, fn in sides:
                    rgb, t, segs = fn()
                    if rep == 0:
                        image[name] = (rgb, segs)
                    else:
                        ms[name].append(t)
            for name in ("b", "c"):
                assert np.array_equal(image[name][0], image["a"][0]) and image[name][1] == image["a"][1], name
            med = {k: statistics.median(v) for k, v in ms.items()}
            say(f"{config} {w}x{h} x {spp} spp {prec}: records {nbytes.value / 1e6:.1f} MB, schedule {schedule}")
            for name, what in (("a", "rt_render_async"), ("b", "session, one step"), ("c", f"session, {len(schedule)} steps")):
                say(f"    ({name}) {what:<20} {med[name]:9.3f} ms [{min(ms[name]):.3f}..{max(ms[name]):.3f}]")
            say(f"    b/a {med['b'] / med['a']:.2f}   c/b {med['c'] / med['b']:.2f}")
        finally:
            r.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
