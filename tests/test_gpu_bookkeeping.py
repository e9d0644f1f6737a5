"""GPU parity for the path loop's wave-uniform bookkeeping (rt_trace_body.hpp): issue()'s fast path (a batch served
whole from the open item) against its slow path, the packed issue state, the slot mask issue() hands the camera
batch, the per-slot "no candidate list" bit, and the once-per-iteration counter update.  None of it may change an
image or a counter.

Bar (tests/test_gpu_sweep_flush.py's): the linear image array_equal, the RGB8 bytes equal, ray_segments and the return
code equal to the CPU oracle's.  On top of it every case's counters are compared with the values the library of the
commit before this change returned on the GPU (tests/golden/bookkeeping_stats.json; tools in the docstring of
measure()): samples, pixels, ray_segments, bounce_iters and direct_sky_samples of every case, which are sums over
pixels and samples and do not depend on which wave traced what; and, for the one-pixel launches (one wave works the
pixel: deterministic), every counter of rt_stats, lane slots and the executed-work counts included.  lane_slots of a
launch of several waves depends on the claim order; there it is checked to be whole waves covering the traced segments.

Shapes: the smallest at which this code can go wrong.
  batch boundaries  spp 1 .. 193 around the 64-lane batch on 1x1, 3x1, 5x3 and 16x8 (fewer pixels than waves, a batch
                    spanning two pixels, a short last batch, fast next to slow calls)
  slots             50 concentric shells, depth 50, 64 spp: stragglers keep all 8 slots busy (issue()'s avail == 0)
  sky at claim      a horizontal camera: direct-sky pixels next to listed ones in one block; depth 0, 1 and 2
  every user        a defocus camera (the issue path without camera batches), ROOT2 / scalar / v1 / v3, fp64,
                    RT_WAVES=5, a row-strided tile, the split, window and items kernels, and rt_render_rays_async on a
                    frame with invalid rays (the `continue` in issue())
"""
import json
import os

import numpy as np
import pytest

import edge_scenes as es
import ray_render_cases as rrc
import rt_mi355x as rt
from rt_mi355x import abi
from oracle_bind import oracle_render

pytestmark = pytest.mark.gpu

SEED = es.SEED
F32 = abi.RT_FLAG_F32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bookkeeping_stats.json")
# sums over pixels and samples: the same whichever wave traced what
SUMS = ("pixels", "samples", "ray_segments", "bounce_iters", "direct_sky_samples")
# ... and what one wave alone determines
ALL = SUMS + ("lane_slots", "box_groups", "filter_groups", "exact_tests", "cone_tests", "camera_exact_tests")


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    monkeypatch.delenv("RT_WAVES", raising=False)
    monkeypatch.delenv("RT_FILTER_OFF", raising=False)


# ---------------------------------------------------------------- scenes
HORIZON = dict(rt.MAIN_CAMERA, center=(13.0, 1.0, 3.0), look_at=(0.0, 1.0, 0.0), view_angle=40.0)


def scene(name, w, h):
    """-> (FlatScene, RtCamera).  s100: random_spheres(100) under the main (pinhole) camera; defocus: the same with a
    defocus disk; horizon: the camera level at y = 1, the upper rows all sky; shells: edge_scenes.concentric."""
    if name == "shells":
        return es.concentric(w, h)
    flat = rrc.scene("s100")
    cam = {"s100": rt.MAIN_CAMERA, "defocus": dict(rt.MAIN_CAMERA, defocus_angle=0.6), "horizon": HORIZON}[name]
    return flat, rt.camera_new_py(w, h, **cam)


# ---------------------------------------------------------------- the cases
def case(scn="s100", w=16, h=8, spp=64, depth=4, flags=F32, tile=None, spi=None, waves=None):
    return dict(scene=scn, w=w, h=h, spp=spp, depth=depth, flags=flags, tile=tile, spi=spi, waves=waves)


FRAMES = [(1, 1), (3, 1), (5, 3), (16, 8)]
SPPS = [1, 63, 64, 65, 100, 127, 128, 129, 193]
CASES = {f"batch-{w}x{h}-{spp}": case(w=w, h=h, spp=spp) for w, h in FRAMES for spp in SPPS}
CASES.update({
    # one-pixel launches whose every counter is recorded
    "one-64": case(w=1, h=1, spp=64, depth=8),
    "one-200": case(w=1, h=1, spp=200, depth=8),
    "slots": case("shells", spp=64, depth=50),
    "slots-3x1": case("shells", w=3, h=1, spp=64, depth=50),
    "sky-d0": case("horizon", depth=0), "sky-d1": case("horizon", depth=1), "sky-d2": case("horizon", depth=2),
    "sky-d2-100": case("horizon", spp=100, depth=2),
    "defocus": case("defocus", spp=65), "defocus-5x3": case("defocus", w=5, h=3, spp=129),
    "root2": case(spp=65, flags=F32 | abi.RT_FLAG_ROOT2),
    "scalar": case(spp=65, flags=F32 | abi.RT_FLAG_MODE_SCALAR),
    "v1": case(spp=65, flags=F32 | abi.RT_FLAG_MODE_VECTORIZED),
    "v3": case(spp=65, flags=F32 | abi.RT_FLAG_MODE_VECTORIZED3),
    "f64": case(spp=65, flags=0), "f64-sky": case("horizon", spp=100, depth=2, flags=0),
    "f64-defocus": case("defocus", w=5, h=3, spp=65, flags=0),
    "waves5": case(spp=129, waves=5), "waves5-sky": case("horizon", spp=65, depth=2, waves=5),
    # rows 1, 3, 5 of 8, columns 2 .. 12
    "strided": case(spp=65, tile=(1, 2, 3, 2, 11)), "strided-sky": case("horizon", spp=65, depth=2, tile=(0, 3, 3, 0, 16)),
    # the sample-parallel kernel: items of 24 samples (a batch spans items of one pixel and of two)
    "split": case(spp=65, spi=24), "split-sky": case("horizon", spp=100, depth=2, spi=24),
    "split-1x1": case(w=1, h=1, spp=193, spi=50), "split-shells": case("shells", w=5, h=3, spp=64, depth=50, spi=16),
})


def _pixels(c):
    if c["tile"] is None:
        return None
    rb, rs, rn, cb, cn = c["tile"]
    return np.array([(rb + i * rs) * c["w"] + cb + j for i in range(rn) for j in range(cn)], np.uint32)


_refs = {}


def reference(name):
    """The oracle's render of a case, once, read-only."""
    if name not in _refs:
        c = CASES[name]
        flat, cam = scene(c["scene"], c["w"], c["h"])
        r = oracle_render(flat, cam, c["depth"], c["spp"], SEED, c["flags"] & ~F32, pixels=_pixels(c),
                          precision="f32" if c["flags"] & F32 else "f64")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[name] = r
    return _refs[name]


def stats_dict(st, fields):
    return {f: int(getattr(st, f)) for f in fields}


def measure(renderer, name):
    """Render a case: ((rgb, linear, RtStats, rc), the counters the golden file holds for it).  The golden file is
    {case: measure(...)[1]} over CASES and RAY_CASES, recorded with the library of the commit before the change."""
    c = CASES[name]
    flat, cam = scene(c["scene"], c["w"], c["h"])
    if c["waves"] is not None:
        os.environ["RT_WAVES"] = str(c["waves"])
    try:
        renderer.seed, renderer.flags = SEED, c["flags"]
        tr = abi.RtTileRange(*c["tile"]) if c["tile"] is not None else None
        got = renderer.render_flat(c["depth"], c["spp"], flat, cam, tile_range=tr, want_linear=True,
                                   samples_per_item=c["spi"])
    finally:
        os.environ.pop("RT_WAVES", None)
    npx = c["w"] * c["h"] if c["tile"] is None else c["tile"][2] * c["tile"][4]
    return got, stats_dict(got[2], ALL if npx == 1 and c["spi"] is None else SUMS)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check_counters(st, rec, want, npx, spp):
    print("counters", rec, "recorded", want)
    assert rec == want
    assert st.pixels == npx and st.samples == npx * spp
    assert st.direct_sky_samples % spp == 0 and st.direct_sky_samples <= st.samples
    # whole waves; a pixel finished at claim time counts its segments and holds no lane
    assert st.lane_slots % 64 == 0 and st.lane_slots >= st.ray_segments - st.direct_sky_samples


@pytest.mark.parametrize("name", list(CASES))
def test_case(renderer, golden, name):
    c = CASES[name]
    (rgb, lin, st, code), rec = measure(renderer, name)
    rgb_o, lin_o, segs_o, rc_o = reference(name)
    assert code == rc_o
    diff = np.argwhere(lin != lin_o)
    assert diff.size == 0, f"{len(diff)} mismatching channels of {lin_o.size}; first pixel {diff[0][0]}"
    np.testing.assert_array_equal(rgb, rgb_o)
    assert st.ray_segments == segs_o
    check_counters(st, rec, golden[name], len(lin_o), c["spp"])
    k = abi.kernel_info(st.kernel_id)
    assert k["T"] == ("float" if c["flags"] & F32 else "double")
    assert bool(abi.RT_KERNEL_SPLIT(st.kernel_id)) == (c["spi"] is not None)
    if c["waves"] is not None:
        assert k["W"] == c["waves"]
    # the camera-batch kernels for the pinhole cameras at depth >= 1, the general issue path for the rest
    assert bool(k["camq"]) == (c["scene"] != "defocus" and c["depth"] >= 1)


def test_sky_pixels_finish_at_claim_time(renderer):
    """The horizon frame holds both kinds of pixel, and only a depth above 1 finishes the sky ones at claim time."""
    for name, direct in (("sky-d0", False), ("sky-d1", False), ("sky-d2", True), ("f64-sky", True), ("split-sky", False)):
        (_, _, st, _), _ = measure(renderer, name)
        c = CASES[name]
        if direct:
            assert 0 < st.direct_sky_samples < st.samples, "direct-sky pixels next to listed ones"
            assert st.cone_tests > 0 and st.camera_exact_tests > 0
        else:
            assert st.direct_sky_samples == 0
        assert st.samples == c["w"] * c["h"] * c["spp"]


# ---------------------------------------------------------------- the window and items kernels
@pytest.mark.parametrize("name", ["batch-5x3-129", "sky-d2-100", "split-shells"])
def test_window_and_items_kernels(renderer, name):
    """A progressive session: a third of the samples, then all (trace_paths_window); then per-pixel counts, a third or
    all, from a second session (trace_paths_items).  Every image is the oracle's at that count."""
    c = CASES[name]
    flat, cam = scene(c["scene"], c["w"], c["h"])
    spp, depth = c["spp"], c["depth"]
    part = max(1, spp // 3)
    refs = {n: oracle_render(flat, cam, depth, n, SEED, 0, precision="f32") for n in (part, spp)}
    renderer.seed, renderer.flags = SEED, F32
    npx = c["w"] * c["h"]
    with renderer.begin_progressive(depth, spp, flat, cam) as s:
        for n in (part, spp):
            rgb, lin, st, code = s.extend(n, want_linear=True)
            np.testing.assert_array_equal(lin, refs[n][1])
            np.testing.assert_array_equal(rgb, refs[n][0])
            assert code == refs[n][3]
        assert st.samples == npx * (spp - part)
    targets = np.where(np.arange(npx) % 3 == 0, spp, part).astype(np.uint32)
    with renderer.begin_progressive(depth, spp, flat, cam) as s:
        rgb, lin, st, code = s.extend_map(targets, want_linear=True)
        assert abi.RT_KERNEL_ITEMS(st.kernel_id) and st.samples == int(targets.sum())
    np.testing.assert_array_equal(lin, np.where((targets == spp)[:, None], refs[spp][1], refs[part][1]))
    np.testing.assert_array_equal(rgb, np.where((targets == spp)[:, None], refs[spp][0], refs[part][0]))


# ---------------------------------------------------------------- caller rays with invalid ones among them
RAY_CASES = {"rays-f32": ("f32", 65, 8), "rays-f64": ("f64", 7, 8)}
BAD = [0, 5, 63, 64, 129]   # the first ray, the ends of the first batch, the last ray


def measure_rays(lib, name):
    prec, spp, depth = RAY_CASES[name]
    o, tgt, d = rrc.ray_set(prec)
    d2 = d.copy()
    d2[BAD[0], 1] = np.nan
    d2[BAD[1]] = 0.0
    d2[BAD[2], 0] = np.inf
    d2[BAD[3]] *= 1e4
    d2[BAD[4], 2] = -np.inf
    r = rt.GpuRenderer(precision=prec, seed=rrc.SEED, lib=lib)
    try:
        got = r.render_rays(depth, spp, o, d2, rrc.scene("s100"), pixel_base=rrc.PIXEL_BASE, want_linear=True)
    finally:
        r.close()
    return got, stats_dict(got[2], SUMS)


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_rays_with_invalid_pixels(lib, golden, name):
    prec, spp, depth = RAY_CASES[name]
    (rgb, lin, st, code), rec = measure_rays(lib, name)
    o, tgt, _ = rrc.ray_set(prec)
    ok = np.ones(rrc.N_PIX, bool)
    ok[BAD] = False
    segs, rc_o = 0, 0
    for p in np.flatnonzero(ok):   # reference A (ray_render_cases.reference_a), the valid pixels only
        r_o, l_o, s, c = oracle_render(rrc.scene("s100"), rrc.degenerate_camera(o[p], tgt[p]), depth, spp, rrc.SEED, 0,
                                       pixels=np.array([rrc.PIXEL_BASE + p], np.uint32), precision=prec, threads=1)
        assert np.array_equal(lin[p], l_o[0]) and np.array_equal(rgb[p], r_o[0]), f"pixel {p}"
        segs += s
        rc_o = max(rc_o, c)
    assert code == rc_o and st.ray_segments == segs
    assert np.isnan(lin[~ok]).all() and (rgb[~ok] == 0).all()
    print("counters", rec, "recorded", golden[name])
    assert rec == golden[name]
    assert st.pixels == rrc.N_PIX and st.samples == (rrc.N_PIX - len(BAD)) * spp and st.direct_sky_samples == 0
    assert abi.RT_KERNEL_RAYS(st.kernel_id)
