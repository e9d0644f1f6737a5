#!/usr/bin/env python3
"""The price and the gain of per-pixel sample counts on one GPU, same process and context, by the method of
tools/progressive_ab.py: a warm-up of each side, then the sides alternating, the median of REPS kernel_ms
(rt_context_collect, HIP events; the item table's copy to the device is inside them).  The wall time of the calls
(the host's plan and staging included) is printed beside it.  Config C's scene, fp32.

(a) The price of the item table and of the class launches: a session extended to the final spp in one step with
    the image, by rt_progressive_extend_async (u) and by a map that is uniform but for one pixel, which holds one
    sample less (m).  Reports m/u.  There is no threshold: the number is the price.
(b) An adaptive run (GpuRenderer.adaptive's policy, 16 -> 512 spp on config C's frame, the tolerance at the median
    of the first error estimate) against a uniform session extended to 512 spp.  Reports the samples traced, the
    steps, kernel_ms and wall time of both, and where the adaptive run's kernel time goes (tracing steps, error
    estimates, the final image).  A third leg (d) runs the same policy planned on the device
    (rt_progressive_refine); its counts must equal the host-driven leg's.  A refine call returns when its selection
    is known and its tracing is enqueued, so the wall time of the call is the step's estimate, selection and
    readback, and the step's kernel_ms less that is its tracing.

The evidence for DESIGN.md §4 "Per-pixel counts" (profiles/adaptive.txt, profiles/adaptive_device.txt).

    python tools/adaptive_ab.py [--reps 7] [--parts a,b] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
import rt_mi355x as rt  # noqa: E402

PRICE_SHAPES = [(1920, 1080, 64), (64, 36, 4096)]   # (width, height, spp)
SPP_MIN, SPP_MAX = 16, 512


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


def price(say, lib, flat, depth, reps):
    for w, h, spp in PRICE_SHAPES:
        cam = rt.camera_new_py(w, h, **rt.MAIN_CAMERA)
        r = rt.GpuRenderer(precision="f32", lib=lib)
        targets = np.full(w * h, spp, np.uint32)
        targets[(h // 2) * w + w // 2] = spp - 1

        def run(use_map):
            with r.begin_progressive(depth, spp, flat, cam) as s:
                t0 = time.perf_counter()
                _, _, st, _ = s.extend_map(targets) if use_map else s.extend(spp)
                return st.kernel_ms, (time.perf_counter() - t0) * 1e3, st.samples

        try:
            res = alternate([("u", lambda: run(False)), ("m", lambda: run(True))], reps)
            say(f"(a) C {w}x{h} x {spp} spp f32, one step with the image")
            for name, what in (("u", "rt_progressive_extend_async"), ("m", "map, one pixel at spp - 1")):
                ms, wall = [x[0] for x in res[name]], [x[1] for x in res[name]]
                say(f"    ({name}) {what:<28} kernel {med(ms):9.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  "
                    f"wall {med(wall):9.3f} ms  samples {res[name][0][2]}")
            say(f"    m/u kernel {med([x[0] for x in res['m']]) / med([x[0] for x in res['u']]):.3f}   "
                f"wall {med([x[1] for x in res['m']]) / med([x[1] for x in res['u']]):.3f}")
        finally:
            r.close()


def gain(say, lib, flat, depth, reps):
    w, h = rt.scenes.CONFIGS["C"][:2]
    cam = rt.camera_new_py(w, h, **rt.MAIN_CAMERA)
    r = rt.GpuRenderer(precision="f32", lib=lib)
    try:
        with r.begin_progressive(depth, SPP_MAX, flat, cam) as s:
            s.extend(SPP_MIN, image=False)
            tol = float(np.median(s.error()))

        def uniform():
            with r.begin_progressive(depth, SPP_MAX, flat, cam) as s:
                t0 = time.perf_counter()
                _, _, st, _ = s.extend(SPP_MAX)
                return {"ms": st.kernel_ms, "wall": (time.perf_counter() - t0) * 1e3, "samples": st.samples}

        def adaptive():
            # GpuRenderer.adaptive's loop, with the kernel time of each kind of call kept apart
            out = {"trace": 0.0, "error": 0.0, "image": 0.0, "samples": 0, "steps": [], "active": []}
            with r.begin_progressive(depth, SPP_MAX, flat, cam) as s:
                t0 = time.perf_counter()
                st = s.extend(SPP_MIN, image=False)
                out["trace"] += st.kernel_ms
                out["samples"] += st.samples
                out["steps"].append(st.kernel_ms)
                while True:
                    err, st = s.error(stats=True)
                    out["error"] += st.kernel_ms
                    counts = s.counts
                    active = (err > tol) & (counts < SPP_MAX)
                    if not active.any():
                        break
                    counts[active] = np.minimum(2 * counts[active], SPP_MAX)
                    st = s.extend_map(counts, image=False)
                    out["trace"] += st.kernel_ms
                    out["samples"] += st.samples
                    out["steps"].append(st.kernel_ms)
                    out["active"].append(int(active.sum()))
                _, _, st, _ = s.snapshot()
                out["image"] = st.kernel_ms
                out["wall"] = (time.perf_counter() - t0) * 1e3
                out["counts"] = s.counts
                out["classes"] = np.unique(out["counts"], return_counts=True)
            out["ms"] = out["trace"] + out["error"] + out["image"]
            return out

        def device():
            out = {"trace": 0.0, "error": 0.0, "image": 0.0, "samples": 0, "steps": [], "active": []}
            with r.begin_progressive(depth, SPP_MAX, flat, cam) as s:
                t0 = time.perf_counter()
                st = s.extend(SPP_MIN, image=False)
                out["trace"] += st.kernel_ms
                out["samples"] += st.samples
                out["steps"].append(st.kernel_ms)
                while True:
                    t1 = time.perf_counter()
                    n_active, _ = s.refine(tol, SPP_MAX)
                    select_ms = (time.perf_counter() - t1) * 1e3
                    st = s.collect()
                    if n_active == 0 and st.kernel_ms == 0.0:   # every candidate at the cap: nothing ran
                        break
                    select_ms = min(select_ms, st.kernel_ms)
                    out["error"] += select_ms
                    if n_active == 0:
                        break
                    out["trace"] += st.kernel_ms - select_ms
                    out["samples"] += st.samples
                    out["steps"].append(st.kernel_ms - select_ms)
                    out["active"].append(n_active)
                _, _, st, _ = s.snapshot()
                out["image"] = st.kernel_ms
                out["wall"] = (time.perf_counter() - t0) * 1e3
                out["counts"] = s.counts
                out["classes"] = np.unique(out["counts"], return_counts=True)
            out["ms"] = out["trace"] + out["error"] + out["image"]
            return out

        res = alternate([("u", uniform), ("a", adaptive), ("d", device)], reps)
        u, a, d = res["u"], res["a"], res["d"]
        assert all(np.array_equal(x["counts"], y["counts"]) for x, y in zip(a, d)), "device and host counts differ"
        assert d[0]["samples"] == a[0]["samples"] and d[0]["active"] == a[0]["active"]
        say(f"(b) C {w}x{h} f32, {SPP_MIN} -> {SPP_MAX} spp, tolerance {tol:.6g} (the median of the first error)")
        say(f"    (u) uniform session to {SPP_MAX}     kernel {med([x['ms'] for x in u]):9.3f} ms  "
            f"wall {med([x['wall'] for x in u]):9.3f} ms  samples {u[0]['samples']}")
        say(f"    (a) adaptive, {len(a[0]['steps']) - 1} refinement steps  kernel {med([x['ms'] for x in a]):9.3f} ms  "
            f"wall {med([x['wall'] for x in a]):9.3f} ms  samples {a[0]['samples']}")
        say(f"        kernel ms: tracing {med([x['trace'] for x in a]):.3f}, error estimates {med([x['error'] for x in a]):.3f}, "
            f"final image {med([x['image'] for x in a]):.3f}")
        say("        per step (first: the uniform one): " +
            ", ".join(f"{med([x['steps'][i] for x in a]):.3f}" for i in range(len(a[0]['steps']))))
        say(f"        active pixels per refinement step: {a[0]['active']}")
        say("        pixels ending at each count: " + ", ".join(f"{n}: {c}" for n, c in zip(*a[0]["classes"])))
        say(f"    samples a/u {a[0]['samples'] / u[0]['samples']:.3f}   kernel a/u "
            f"{med([x['ms'] for x in a]) / med([x['ms'] for x in u]):.3f}   wall a/u "
            f"{med([x['wall'] for x in a]) / med([x['wall'] for x in u]):.3f}")
        say(f"    (d) device-planned, {len(d[0]['steps']) - 1} refinement steps  kernel {med([x['ms'] for x in d]):9.3f} ms  "
            f"wall {med([x['wall'] for x in d]):9.3f} ms  samples {d[0]['samples']}  (counts equal to (a)'s)")
        say(f"        kernel ms: tracing {med([x['trace'] for x in d]):.3f}, estimates and selection "
            f"{med([x['error'] for x in d]):.3f}, final image {med([x['image'] for x in d]):.3f}")
        say("        per step (first: the uniform one): " +
            ", ".join(f"{med([x['steps'][i] for x in d]):.3f}" for i in range(len(d[0]['steps']))))
        say(f"        active pixels per refinement step: {d[0]['active']}")
        for name, other in (("u", u), ("a", a)):
            say(f"    kernel d/{name} {med([x['ms'] for x in d]) / med([x['ms'] for x in other]):.3f}   wall d/{name} "
                f"{med([x['wall'] for x in d]) / med([x['wall'] for x in other]):.3f}")
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = rt.load_library()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"{lib.rt_version().decode()}  reps {args.reps} (median; sides alternating after one warm-up of each)")
    flat = rt.scenes.config_scene("C").flatten()
    depth = rt.scenes.CONFIGS["C"][4]
    if "a" in args.parts.split(","):
        price(say, lib, flat, depth, args.reps)
    if "b" in args.parts.split(","):
        gain(say, lib, flat, depth, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
