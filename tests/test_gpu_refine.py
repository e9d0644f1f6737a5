"""rt_progressive_refine: the doubling policy's estimate, selection and item table on the device (refine_select,
refine_scan, refine_scatter, refine_expand in front of trace_paths_items; finish_window_list over device lists).

Bar: ==.  Results are defined by the counts alone, so the device path must give exactly the counts and the image
of the host-driven policy (GpuRenderer.adaptive(plan="host")) and of the oracle's replay of it.  Shapes: a few
thousand pixels at most on random_spheres(100) at depth 8.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt_mi355x as rt
from rt_mi355x import abi
from test_gpu_adaptive import (DEPTH, F32, MI355X_WAVES, SEED, cam_for, open_session, oracle_map, plan, replay,
                               scene_100, tile_pixels)  # noqa: F401  (scene_100 is a fixture)

pytestmark = pytest.mark.gpu

COMPACTION_BLOCK = 256   # kRefineBlock (rt_trace.hpp): candidates per workgroup of the compaction kernels


def test_compaction_block_is_the_kernels():
    assert f"kRefineBlock = {COMPACTION_BLOCK};" in abi.kernel_source_text()


def oracle_err(key, flat, cam, counts, flags, tile=None):
    """progressive_error's estimate from the oracle: max over channels of |lin(n) - lin(n // 2)|, inf below 2."""
    counts = np.asarray(counts)
    full = oracle_map(key, flat, cam, DEPTH, counts, flags, tile)[1]
    half = oracle_map(key, flat, cam, DEPTH, counts // 2, flags, tile)[1]
    err = np.abs(full - half).max(axis=1)
    err[counts < 2] = np.inf
    return err


def replay_steps(key, flat, cam, flags, spp_min, spp_max, tolerance, tile=None, strict=True, probe=False):
    """The policy with the oracle, step by step: [counts after extend(spp_min), counts after step 1, ...].
    strict: no estimate of the run equals the tolerance (every tolerance that was picked from the estimates)."""
    n = len(tile_pixels(cam, tile))
    counts, out = np.full(n, spp_min, np.uint32), []
    while True:
        out.append(counts.copy())
        err = oracle_err(key, flat, cam, counts, flags, tile)
        tie = ((err == tolerance) & (counts < spp_max)).any()       # at the cap no estimate decides anything
        if probe and tie:
            return None
        if strict:
            assert not tie
        active = (err > tolerance) & (counts < spp_max)
        if not active.any():
            return out
        counts[active] = np.minimum(2 * counts[active], spp_max)


def middle(err, frac=0.5):
    """The midpoint between the lower middle estimate and the next distinct estimate above it: np.median of an even
    number of estimates without a tie in the middle; with an odd number, or pixels that share the middle value (sky
    pixels of one row do), the nearest value above the median that no estimate sits on.  frac: another point of that
    gap (fp32 estimates are few enough for a later step's estimate to sit on the midpoint)."""
    e = np.sort(err)
    lo = e[(len(e) - 1) // 2]
    return float(lo + (e[e > lo][0] - lo) * frac)


def first_median(key, flat, cam, flags, spp, tile=None):
    """The median of the estimate at `spp` everywhere; no estimate sits on it."""
    n = len(tile_pixels(cam, tile))
    err = oracle_err(key, flat, cam, np.full(n, spp, np.uint32), flags, tile)
    tol = middle(err)
    assert np.isfinite(tol) and not (err == tol).any()
    return tol


def chain_median(key, flat, cam, flags, spp_min, spp_max, tile=None):
    """For starts below a few samples, where the reference's reduction of a partial chunk (quirk Q3) makes most
    estimates one and the same number (2.0 at 2 samples, 1.0 at 4): the middle of the estimates at the first count
    of the doubling chain at which they are not mostly one number and none sits on it.  replay_steps then asserts
    the latter of every step."""
    n, c = len(tile_pixels(cam, tile)), spp_min
    while c < spp_max:
        err = oracle_err(key, flat, cam, np.full(n, c, np.uint32), flags, tile)
        if np.isfinite(err).all() and 2 * len(np.unique(err)) > n:
            for frac in (1 / 2, 1 / 3, 2 / 3, 1 / 5):
                tol = middle(err, frac)
                if replay_steps(key, flat, cam, flags, spp_min, spp_max, tol, tile, probe=True) is not None:
                    return tol
        c *= 2
    raise AssertionError("every count of the chain has an estimate on its median")


def run_session(s, tol, spp_min, spp_max, between=None):
    """extend(spp_min), then refine until it returns 0: ([(n_active, n_samples, RtStats)], total RtStats fields)."""
    s.extend(spp_min, image=False)
    steps = []
    while True:
        na, ns = s.refine(tol, spp_max)
        st = s.collect()
        steps.append((na, ns, st))
        if na == 0:
            return steps
        if between:
            between()


# ---- 1. the whole run, against the oracle and against the host-driven policy ----
@pytest.mark.parametrize("flags", [0, F32])
def test_whole_run(renderer, scene_100, flags):
    cam, key = cam_for(16, 9), ("err", flags)
    want, tol, steps = replay(key, scene_100, cam, flags, 8, 64)
    assert len(np.unique(want)) >= 2 and steps >= 1
    rgb_o, _, segs_o, rc_o = oracle_map(key, scene_100, cam, DEPTH, want, flags)
    assert rc_o == abi.RT_OK
    renderer.seed, renderer.flags = SEED, flags
    img_d, counts_d, stat_d = renderer.adaptive(DEPTH, 8, 64, tol, scene_100, cam, plan="device")
    assert img_d.shape == (9, 16, 3) and img_d.dtype == np.uint8
    assert counts_d.shape == (9, 16) and counts_d.dtype == np.uint32
    np.testing.assert_array_equal(counts_d.reshape(-1), want)
    np.testing.assert_array_equal(img_d.reshape(-1, 3), rgb_o)
    assert stat_d.samples == int(counts_d.sum()) and stat_d.ray_segments == segs_o
    img_h, counts_h, stat_h = renderer.adaptive(DEPTH, 8, 64, tol, scene_100, cam, plan="host")
    np.testing.assert_array_equal(counts_d, counts_h)
    np.testing.assert_array_equal(img_d, img_h)
    assert (stat_h.samples, stat_h.ray_segments) == (stat_d.samples, stat_d.ray_segments)
    # fewer reductions ran: the candidates once per step, not the whole frame twice
    assert 0 < stat_d.bounce_iters < stat_h.bounce_iters, (stat_d.bounce_iters, stat_h.bounce_iters)


# ---- 2. a cap off the doubling grid ----
def test_cap_off_the_grid(renderer, scene_100):
    """8 -> 50: the last step is 32 -> 50, and the call after it runs nothing: no estimate at 50."""
    cam, key, flags = cam_for(16, 9), ("err", F32), F32
    tol = first_median(key, scene_100, cam, flags, 8)
    want = replay_steps(key, scene_100, cam, flags, 8, 50, tol)
    assert (want[-1] == 50).any() and set(np.unique(want[-1])) <= {8, 16, 32, 50}
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        steps = run_session(s, tol, 8, 50)
        assert len(steps) == len(want)
        for k, (na, ns, st) in enumerate(steps[:-1]):
            grew = want[k + 1] != want[k]
            assert na == int(grew.sum()) and ns == int((want[k + 1] - want[k]).sum()) == st.samples
            assert abi.RT_KERNEL_SPLIT(st.kernel_id) and abi.RT_KERNEL_ITEMS(st.kernel_id) and st.pixels == 144
        assert steps[-2][1] == 18 * steps[-2][0]                     # 32 -> 50
        na, ns, st = steps[-1]
        assert (na, ns, st.samples, st.pixels, st.bounce_iters, st.kernel_id) == (0, 0, 0, 0, 0, 0)
        np.testing.assert_array_equal(s.counts, want[-1])
        rgb, lin, st, rc = s.snapshot(None, want_linear=True)
        rgb_o, lin_o, _, rc_o = oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)
        np.testing.assert_array_equal(lin, lin_o)
        np.testing.assert_array_equal(rgb, rgb_o)
        assert rc == rc_o and st.samples == 0


# ---- 3. small and odd starts ----
def test_start_at_one_sample(renderer, scene_100):
    """spp_min = 1: the estimate is +inf, so every pixel is active once; from 2 on the estimates decide.  (At 1
    sample the reference's reduction reads its other buffer, quirk Q3, and most estimates at 2 are exactly 2.0: the
    tolerance is chain_median's, and the replay asserts that no estimate at any step equals it.)"""
    cam, key, flags, n = cam_for(16, 9), ("err", F32), F32, 144
    tol = chain_median(key, scene_100, cam, flags, 1, 16)
    want = replay_steps(key, scene_100, cam, flags, 1, 16, tol)
    assert (want[1] == 2).all() and len(np.unique(want[-1])) >= 2
    with open_session(renderer, scene_100, cam, 16, flags) as s:
        steps = run_session(s, tol, 1, 16)
        assert steps[0][:2] == (n, n)
        assert [x[0] for x in steps[:-1]] == [int((b != a).sum()) for a, b in zip(want, want[1:])]
        np.testing.assert_array_equal(s.counts, want[-1])
        lin = s.snapshot(None, want_linear=True)[1]
        np.testing.assert_array_equal(lin, oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)[1])


def test_start_at_three_samples(renderer, scene_100):
    """spp_min = 3: the first half count is 1, and 6 // 2 == 3, 12 // 2 == 6 keep the kept values exact."""
    cam, key, flags = cam_for(16, 9), ("err", F32), F32
    tol = chain_median(key, scene_100, cam, flags, 3, 24)
    want = replay_steps(key, scene_100, cam, flags, 3, 24, tol)
    assert len(want) >= 3
    renderer.seed, renderer.flags = SEED, flags
    img, counts, stat = renderer.adaptive(DEPTH, 3, 24, tol, scene_100, cam, plan="device")
    np.testing.assert_array_equal(counts.reshape(-1), want[-1])
    rgb_o, _, segs_o, _ = oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)
    np.testing.assert_array_equal(img.reshape(-1, 3), rgb_o)
    assert stat.samples == int(want[-1].sum()) and stat.ray_segments == segs_o


# ---- 4. nothing or everything active ----
def test_nothing_active(renderer, scene_100):
    cam, key, flags = cam_for(16, 9), ("err", F32), F32
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        s.extend(8, image=False)
        assert s.refine(1e30, 64) == (0, 0)
        st = s.collect()
        assert (st.samples, st.ray_segments) == (0, 0) and not abi.RT_KERNEL_ITEMS(st.kernel_id)
        assert s.refine_items()[0] == 0 and s.refine_items()[1].shape == (0, 4)
        assert (s.counts == 8).all()
        rgb, lin, st, rc = s.snapshot(None, want_linear=True)
        rgb_o, lin_o, _, rc_o = oracle_map(key, scene_100, cam, DEPTH, np.full(144, 8), flags)
        np.testing.assert_array_equal(lin, lin_o)
        np.testing.assert_array_equal(rgb, rgb_o)
        assert rc == rc_o
        assert s.refine(1e30, 64) == (0, 0)                          # converged stays converged


def test_everything_active(renderer, scene_100):
    """A tolerance of 0: only an estimate of exactly 0 stops a pixel."""
    cam, key, flags = cam_for(16, 9), ("err", F32), F32
    want = replay_steps(key, scene_100, cam, flags, 8, 32, 0.0, strict=False)
    renderer.seed, renderer.flags = SEED, flags
    img, counts, stat = renderer.adaptive(DEPTH, 8, 32, 0.0, scene_100, cam, plan="device")
    np.testing.assert_array_equal(counts.reshape(-1), want[-1])
    np.testing.assert_array_equal(img.reshape(-1, 3), oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)[0])
    assert stat.samples == int(want[-1].sum())


# ---- 5. compaction across blocks ----
def stepwise_against_the_plan(s, lib, want, tol, spp_max, flags):
    """Refine until 0; after each step the device's item table is the host plan's for the counts before and after
    it (items, order, S) and the counts are the replay's."""
    for k in range(len(want)):
        before = s.counts
        np.testing.assert_array_equal(before, want[k])
        na, ns = s.refine(tol, spp_max)
        s.collect()
        after = s.counts
        S, items = s.refine_items()
        S_h, items_h = plan(lib, before, after, MI355X_WAVES[flags])
        assert S == S_h
        np.testing.assert_array_equal(items[:, :3], items_h)
        assert not items[:, 3].any()
        if na == 0:
            assert k == len(want) - 1 and len(items) == 0
            return
        np.testing.assert_array_equal(after, want[k + 1])
        assert na == int((after != before).sum()) and ns == int((after - before).sum())
    raise AssertionError("the run goes on past the replay's last step")


def test_compaction_across_blocks(renderer, lib, scene_100):
    """97x43 = 4171 pixels: 17 compaction blocks, the last of 75.  4 -> 16 with chain_median's tolerance (the
    estimates at 4 are degenerate, see there), so the later steps compact a list that spans the blocks; then 8 -> 16
    with the middle of its first estimate, which compacts the whole frame's identity list into two ragged halves."""
    cam, key, flags = cam_for(97, 43), ("blocks",), F32
    n = 97 * 43
    assert n > 2 * COMPACTION_BLOCK and n % COMPACTION_BLOCK != 0 and COMPACTION_BLOCK <= 1024
    tol = chain_median(key, scene_100, cam, flags, 4, 16)
    want = replay_steps(key, scene_100, cam, flags, 4, 16, tol)
    assert len(want) >= 3
    grew = [w1 != w0 for w0, w1 in zip(want, want[1:])]
    assert int(grew[0].sum()) > 2 * COMPACTION_BLOCK                 # the second step's candidates: a long list
    assert 0 < int(grew[1].sum()) < int(grew[0].sum())               # ... of which some stop and some go on
    with open_session(renderer, scene_100, cam, 16, flags) as s:
        s.extend(4, image=False)
        stepwise_against_the_plan(s, lib, want, tol, 16, flags)
        rgb = s.snapshot(None)[0]
        np.testing.assert_array_equal(rgb, oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)[0])
    tol = chain_median(key, scene_100, cam, flags, 8, 16)
    want = replay_steps(key, scene_100, cam, flags, 8, 16, tol)
    assert len(want) == 2 and COMPACTION_BLOCK < int((want[1] != want[0]).sum()) < n - COMPACTION_BLOCK
    with open_session(renderer, scene_100, cam, 16, flags) as s:
        s.extend(8, image=False)
        stepwise_against_the_plan(s, lib, want, tol, 16, flags)
        rgb = s.snapshot(None)[0]
        np.testing.assert_array_equal(rgb, oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)[0])


# ---- 6. several items per pixel ----
def test_several_items_per_pixel(renderer, lib, scene_100):
    """4x3, 256 -> 4096: the steps' windows are dealt into items of a multiple of 128 samples, several per pixel."""
    cam, key, flags, n = cam_for(4, 3), ("zero", F32), F32, 12
    err = oracle_err(key, scene_100, cam, np.full(n, 256, np.uint32), flags)
    e = np.unique(err)
    want = None
    for tol in (e[:-1] + e[1:]) / 2:                                 # between two estimates of the oracle
        if (err == tol).any():
            continue
        w = replay_steps(key, scene_100, cam, flags, 256, 4096, float(tol))
        if len(w) >= 3 and (w[-1] < 4096).sum() >= 2:
            want = w
            break
    assert want is not None, "no tolerance between the oracle's estimates gives two steps and two early pixels"
    with open_session(renderer, scene_100, cam, 4096, flags) as s:
        s.extend(256, image=False)
        for k in range(len(want) - 1):
            na, ns = s.refine(float(tol), 4096)
            assert na == int((want[k + 1] != want[k]).sum()) and ns == int((want[k + 1] - want[k]).sum())
            S, items = s.refine_items()
            S_h, items_h = plan(lib, want[k], want[k + 1], MI355X_WAVES[flags])
            assert S == S_h and S % 128 == 0 and len(items) > na
            assert (np.bincount(items[:, 0], minlength=n)[want[k + 1] != want[k]] > 1).all()
            np.testing.assert_array_equal(items[:, :3], items_h)
        assert s.refine(float(tol), 4096) == (0, 0)
        st = s.collect()
        assert st.samples == int((want[-1] - 256).sum())
        np.testing.assert_array_equal(s.counts, want[-1])
        rgb, lin, _, rc = s.snapshot(None, want_linear=True)
        rgb_o, lin_o, _, rc_o = oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)
        np.testing.assert_array_equal(lin, lin_o)
        np.testing.assert_array_equal(rgb, rgb_o)
        assert rc == rc_o


# ---- 7. a row-strided tile ----
def test_row_strided_tile(renderer, scene_100):
    """Rows 1, 4, 7 and columns 5..8 of 16x9: pixels, lists and items are in the range's compact order."""
    cam, key, flags = cam_for(16, 9), ("strided",), F32
    tile = abi.RtTileRange(1, 3, 3, 5, 4)
    tol = first_median(key, scene_100, cam, flags, 8, tile)
    want = replay_steps(key, scene_100, cam, flags, 8, 64, tol, tile)
    assert len(want) >= 2 and len(np.unique(want[-1])) >= 2
    with open_session(renderer, scene_100, cam, 64, flags, tile=tile) as s:
        s.extend(8, image=False)
        for k in range(len(want) - 1):
            na, _ = s.refine(tol, 64)
            items = s.refine_items()[1]
            np.testing.assert_array_equal(items[:, 0], np.flatnonzero(want[k + 1] != want[k]))
            assert na == len(items)
        assert s.refine(tol, 64) == (0, 0)
        s.collect()
        np.testing.assert_array_equal(s.counts, want[-1])
        rgb, lin, _, rc = s.snapshot(None, want_linear=True)
        rgb_o, lin_o, _, rc_o = oracle_map(key, scene_100, cam, DEPTH, want[-1], flags, tile)
        np.testing.assert_array_equal(lin, lin_o)
        np.testing.assert_array_equal(rgb, rgb_o)


# ---- 8. interleaving and refusals ----
def refused(lib, rc, code):
    assert rc == code, (rc, lib.rt_last_error())
    assert b"rt_progressive_refine" in lib.rt_last_error(), lib.rt_last_error()


def c_refine(lib, ctx, tol, spp_max):
    na, ns = ctypes.c_uint64(), ctypes.c_uint64()
    return lib.rt_progressive_refine(ctx, tol, spp_max, None, ctypes.byref(na), ctypes.byref(ns))


def test_interleaved_with_the_other_calls(renderer, scene_100):
    """Two steps, then counts, a snapshot at earlier counts, the error estimate and a host map all agree with the
    oracle; after the host map has traced, refine is refused."""
    cam, key, flags, n = cam_for(16, 9), ("err", F32), F32, 144
    lib, ctx = renderer.lib, renderer.ctx
    tol = first_median(key, scene_100, cam, flags, 8)
    want = replay_steps(key, scene_100, cam, flags, 8, 64, tol)
    assert len(want) >= 3
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        s.extend(8, image=False)
        assert s.refine(tol, 64)[0] > 0
        refused(lib, c_refine(lib, ctx, tol * 2, 64), abi.RT_ERR_INVALID)      # another tolerance
        refused(lib, c_refine(lib, ctx, tol, 32), abi.RT_ERR_INVALID)          # another cap
        refused(lib, c_refine(lib, ctx, float("nan"), 64), abi.RT_ERR_INVALID)
        assert s.refine(tol, 64)[0] > 0
        s.collect()
        counts = s.counts
        np.testing.assert_array_equal(counts, want[2])
        lin = s.snapshot(np.full(n, 8, np.uint32), want_linear=True)[1]
        np.testing.assert_array_equal(lin, oracle_map(key, scene_100, cam, DEPTH, np.full(n, 8), flags)[1])
        lin = s.snapshot(None, want_linear=True)[1]
        np.testing.assert_array_equal(lin, oracle_map(key, scene_100, cam, DEPTH, counts, flags)[1])
        np.testing.assert_array_equal(s.error(), oracle_err(key, scene_100, cam, counts, flags))
        np.testing.assert_array_equal(s.counts, counts)
        target = counts.copy()
        target[::5] += 1
        rgb, lin, st, rc = s.extend_map(target, want_linear=True)
        np.testing.assert_array_equal(lin, oracle_map(key, scene_100, cam, DEPTH, target, flags)[1])
        assert st.samples == int((target - counts).sum())
        np.testing.assert_array_equal(s.counts, target)
        refused(lib, c_refine(lib, ctx, tol, 64), abi.RT_ERR_UNSUPPORTED)
        lin = s.snapshot(None, want_linear=True)[1]                  # the host path again
        np.testing.assert_array_equal(lin, oracle_map(key, scene_100, cam, DEPTH, target, flags)[1])


def test_refusals(renderer, scene_100):
    cam, flags, n = cam_for(16, 9), F32, 144
    lib, ctx = renderer.lib, renderer.ctx
    renderer.set_scene(scene_100)
    refused(lib, c_refine(lib, ctx, 0.1, 64), abi.RT_ERR_INVALID)              # no session
    s_, n_ = ctypes.c_uint32(), ctypes.c_uint64()
    refused(lib, lib.rt_progressive_refine_items(ctx, ctypes.byref(s_), ctypes.byref(n_), None, 0), abi.RT_ERR_INVALID)
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        refused(lib, c_refine(lib, ctx, 0.1, 64), abi.RT_ERR_INVALID)          # no sample yet
        s.extend(8, image=False)
        refused(lib, c_refine(lib, ctx, 0.1, 65), abi.RT_ERR_INVALID)          # above the capacity
        refused(lib, c_refine(lib, ctx, 0.1, 7), abi.RT_ERR_INVALID)           # below the current count
        refused(lib, lib.rt_progressive_refine(ctx, 0.1, 64, None, None, None), abi.RT_ERR_INVALID)
        target = np.full(n, 8, np.uint32)
        target[3] = 9
        s.extend_map(target, image=False)                            # non-uniform by hand
        refused(lib, c_refine(lib, ctx, 0.1, 64), abi.RT_ERR_UNSUPPORTED)
        np.testing.assert_array_equal(s.counts, target)


def test_render_between_steps(renderer, scene_100):
    """rt_render_async of another camera and seed between the steps shares the scratch, the counters and the
    camera tables: the run's counts and image are unchanged, and so is the render."""
    cam, key, flags = cam_for(16, 9), ("err", F32), F32
    other_cam = cam_for(4, 3, center=(13.0, 3.0, -8.0))
    tol = first_median(key, scene_100, cam, flags, 8)
    want = replay_steps(key, scene_100, cam, flags, 8, 64, tol)
    renderer.seed, renderer.flags = 22, flags
    alone = renderer.render_flat(DEPTH, 96, scene_100, other_cam, want_linear=True)[1]
    others = []

    def between():
        renderer.seed = 22
        others.append(renderer.render_flat(DEPTH, 96, scene_100, other_cam, want_linear=True)[1])
        renderer.seed = SEED

    with open_session(renderer, scene_100, cam, 64, flags) as s:
        steps = run_session(s, tol, 8, 64, between)
        assert len(steps) == len(want) and len(others) == len(want) - 1
        np.testing.assert_array_equal(s.counts, want[-1])
        lin = s.snapshot(None, want_linear=True)[1]
        np.testing.assert_array_equal(lin, oracle_map(key, scene_100, cam, DEPTH, want[-1], flags)[1])
    for o in others:
        np.testing.assert_array_equal(o, alone)


# ---- 9. CLI ----
def test_cli_device_plan(tmp_path):
    """rt-render --adaptive ... --device-plan writes byte for byte the files it writes without --device-plan, and
    prints the same step lines."""
    cli = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-ray-tracing_amd", "bin", "rt-render")
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(rt.scenes.three_spheres()))
    base = [cli, "--width", "16", "--height", "9", "--spp", "64", "--bounces", "8", "--f32", "--adaptive", "0.02",
            "--spp-min", "8"]
    outs = []
    for name, extra in (("h", []), ("d", ["--device-plan"])):
        args = base + ["--count-map", f"{name}_counts.ppm", "--out", f"{name}.ppm"] + extra
        r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("Adaptive: ")])
    assert len(outs[0]) >= 2 and outs[0] == outs[1]
    assert (tmp_path / "h.ppm").read_bytes() == (tmp_path / "d.ppm").read_bytes()
    assert (tmp_path / "h_counts.ppm").read_bytes() == (tmp_path / "d_counts.ppm").read_bytes()
    bad = subprocess.run(base[:-4] + ["--device-plan"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--adaptive" in bad.stderr
