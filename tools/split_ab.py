#!/usr/bin/env python3
"""Sample-parallel A/B on one GPU, same process and context: rt_render_async against rt_render_split_async
(auto plan) on launches with fewer pixels than the chip has waves, alternating after a warm-up of both.
Reports kernel_ms from rt_context_collect (HIP events; trace + finish for the split side) as the median of
REPS repetitions, and checks that both sides wrote the same image.  The evidence for DESIGN.md §4
"Sample-parallel launches" (profiles/sample_parallel.txt).

    python tools/split_ab.py [--reps 7] [--factors 4,8,16] [--out FILE]

--factors: also time the split with S planned for that many items per resident wave (the auto plan's
kSplitItemsPerWave is 8), forced through samples_per_item, at each shape.
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

# (config scene, width, height, spp, precision)
SHAPES = [("C", 16, 9, 65536, "f32"), ("C", 64, 36, 4096, "f32"), ("C", 1, 1, 1 << 20, "f32"),
          ("C", 240, 135, 512, "f32"), ("E", 16, 9, 8192, "f32"), ("C", 16, 9, 65536, "f64")]
CUS = 256   # MI355X


def plan_for(factor, n_pixels, spp, waves):
    """rt_split_plan's rule with `factor` items per resident wave (csrc/rt_split_plan.hpp)."""
    per_pixel = 1 if n_pixels >= waves else -(-factor * waves // n_pixels)
    S = -(-(-(-spp // per_pixel)) // 128) * 128
    return spp if S >= spp else S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--factors", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="", help="indices into SHAPES, comma separated (default: all)")
    args = ap.parse_args()
    factors = [int(f) for f in args.factors.split(",") if f]
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")] if args.shapes else SHAPES
    lib = rt.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"{lib.rt_version().decode()}  reps {args.reps} (median kernel_ms; alternating unsplit / split after one warm-up of each)")
    scenes = {}
    for config, w, h, spp, prec in shapes:
        flat = scenes.setdefault(config, rt.scenes.config_scene(config).flatten())
        depth = rt.scenes.CONFIGS[config][4]
        cam = rt.camera_new_py(w, h, **rt.MAIN_CAMERA)
        r = rt.GpuRenderer(precision=prec, lib=lib)
        try:
            waves = CUS * 4 * (5 if prec == "f32" else 4)
            sides = [("unsplit", None), ("auto", 0)] + [(f"x{f}", plan_for(f, w * h, spp, waves)) for f in factors]
            image, ms, info = {}, {k: [] for k, _ in sides}, {}
            for rep in range(args.reps + 1):   # rep 0: warm-up
                for name, S in sides:
                    if S is not None and S >= spp:
                        continue   # a one-item plan: nothing to split
                    rgb, _, st, rc = r.render_flat(depth, spp, flat, cam, samples_per_item=S)
                    assert rc == 0
                    if rep == 0:
                        image[name] = rgb
                        info[name] = (abi.kernel_name(st.kernel_id), st.ray_segments, st.bounce_iters)
                    else:
                        ms[name].append(st.kernel_ms)
            base = statistics.median(ms["unsplit"])
            say(f"{config} {w}x{h} x {spp} spp {prec}: unsplit {base:.3f} ms [{min(ms['unsplit']):.3f}..{max(ms['unsplit']):.3f}]  {info['unsplit'][0]}")
            for name, S in sides[1:]:
                if not ms[name]:
                    say(f"    {name:>7}: plan is one item per pixel")
                    continue
                assert np.array_equal(image[name], image["unsplit"]) and info[name][1:] == info["unsplit"][1:], name
                m = statistics.median(ms[name])
                s_txt = "plan" if S == 0 else f"S={S}"
                if S == 0:
                    s_, n_ = abi.u32(), abi.u64()
                    lib.rt_split_plan(w * h, spp, waves, ctypes.byref(s_), ctypes.byref(n_))
                    s_txt = f"S={s_.value} ({n_.value} items)"
                say(f"    {name:>7}: {m:.3f} ms [{min(ms[name]):.3f}..{max(ms[name]):.3f}]  unsplit/split {base / m:.2f}  {s_txt}  {info[name][0]}")
        finally:
            r.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
