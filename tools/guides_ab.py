#!/usr/bin/env python3
"""What the guide buffers cost beside the render they accompany, on one GPU, same process and context, by the
method of tools/adaptive_ab.py: a warm-up of each side, then the sides alternating, the median of REPS kernel_ms
(rt_context_collect, HIP events).  Config C's frame (1920x1080, 500 spheres), fp32 and fp64, at 16 and 512 spp:

    (g) rt_render_guides_async, all four outputs   (guide_pixels: the primary rays and first hits alone)
    (r) rt_render_async at the same frame, spp and 50 bounces

Reports g/r.  The one condition (DESIGN.md §4 "Guide buffers"): the guide pass takes less kernel time than the
render, whose segments it traces a subset of, with no scatter and no replay.  The script also checks, at the
sizes it times, that the guides' samples and segments are pixels x spp and that their coverage is that of a
frame with both sky and spheres in it.

    python tools/guides_ab.py [--reps 7] [--out FILE]
"""
import argparse
import os
import statistics
import sys


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
import rt_mi355x as rt  # noqa: E402

SPPS = (16, 512)


def med(v):
    return statistics.median(v)


def alternate(sides, reps):
    """{name: [result per rep]} after one warm-up of each side, the sides alternating."""
    out = {k: [] for k, _ in sides}
    for rep in range(reps + 1):
        for name, fn in sides:
            res = fn()
            if rep:
                out[name].append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = rt.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"{lib.rt_version().decode()}  reps {args.reps} (median; sides alternating after one warm-up of each)")
    w, h, _, _, depth = rt.scenes.CONFIGS["C"]
    flat = rt.scenes.config_scene("C").flatten()
    cam = rt.camera_new_py(w, h, **rt.MAIN_CAMERA)
    ok = True
    for prec in ("f32", "f64"):
        r = rt.GpuRenderer(precision=prec, lib=lib)
        try:
            for spp in SPPS:
                def guides():
                    out, st, _ = r.guides_flat(spp, flat, cam)
                    assert st.samples == st.ray_segments == w * h * spp and st.bounce_iters == 0
                    return st.kernel_ms, float(out["coverage"].mean()), rt.abi.kernel_name(st.kernel_id)

                def render():
                    _, _, st, _ = r.render_flat(depth, spp, flat, cam)
                    return st.kernel_ms, st.ray_segments, rt.abi.kernel_name(st.kernel_id)

                res = alternate([("g", guides), ("r", render)], args.reps)
                g, rr = [x[0] for x in res["g"]], [x[0] for x in res["r"]]
                cov = res["g"][0][1]
                assert 0.0 < cov < 1.0 and len({x[1] for x in res["g"]}) == 1
                say(f"C {w}x{h} x {spp} spp {prec}, {depth} bounces")
                say(f"    (g) {res['g'][0][2]:<40} kernel {med(g):9.3f} ms [{min(g):.3f}..{max(g):.3f}]  "
                    f"{w * h * spp / med(g) / 1e3:9.1f} Msamples/s  mean coverage {cov:.4f}")
                say(f"    (r) {res['r'][0][2]:<40} kernel {med(rr):9.3f} ms [{min(rr):.3f}..{max(rr):.3f}]  "
                    f"segments per sample {res['r'][0][1] / (w * h * spp):.3f}")
                say(f"    g/r kernel {med(g) / med(rr):.3f}")
                ok = ok and med(g) < med(rr)
        finally:
            r.close()
    say("the guide pass takes less kernel time than the render at every point: " + ("yes" if ok else "NO"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
