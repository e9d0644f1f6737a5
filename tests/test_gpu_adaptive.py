"""Per-pixel sample counts in progressive sessions (rt_progressive_extend_map_async / _snapshot_map_async /
_counts / _error_async: trace_paths_items over an item table, finish_window_list per distinct count, the
element-wise error kernel) and the adaptive sampler built on them, against the CPU oracle.

Bar: 0 ulp.  Pixel p at n_p samples equals oracle_render's at spp = n_p for that pixel: the oracle is called once
per distinct count with that class's pixel list.  The shapes are a few pixels by at most a few thousand samples on
random_spheres(100) at depth 8 unless a test says otherwise.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt_mi355x as rt
from rt_mi355x import abi
from oracle_bind import oracle_render

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
F32 = abi.RT_FLAG_F32
DEPTH = 8
U32P = ctypes.POINTER(ctypes.c_uint32)
MI355X_WAVES = {F32: 256 * 4 * 5, 0: 256 * 4 * 4}   # resident waves of the sample-parallel kernels (test_many_items)


def cam_for(w, h, **kw):
    return rt.camera_new_py(w, h, **dict(rt.MAIN_CAMERA, **kw))


@pytest.fixture(scope="module")
def scene_100():
    return rt.scenes.random_spheres(100).flatten()


def tile_pixels(cam, tile=None):
    """Global pixel indices of a tile range (None: the whole image), in the output's order."""
    if tile is None:
        return np.arange(cam.image_width * cam.image_height, dtype=np.uint32)
    rows = tile.row_begin + np.arange(tile.row_count, dtype=np.int64) * tile.row_step
    cols = tile.col_begin + np.arange(tile.col_count, dtype=np.int64)
    return (rows[:, None] * cam.image_width + cols[None, :]).reshape(-1).astype(np.uint32)


_refs = {}


def oracle_class(key, flat, cam, depth, spp, flags, pixels, seed=SEED):
    """oracle_render of one pixel list at one count, computed once per (key, count, list) and left unchanged."""
    k = key + (spp, pixels.tobytes())
    if k not in _refs:
        r = oracle_render(flat, cam, depth, spp, seed, 0, pixels=pixels, precision="f32" if flags & F32 else "f64")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[k] = r
    return _refs[k]


def oracle_map(key, flat, cam, depth, counts, flags, tile=None, seed=SEED):
    """The oracle at per-pixel counts: (rgb [n,3], lin [n,3], segments, rc), one oracle_render per distinct
    count over that class's pixels.  Pixels with count 0 keep NaN / 0 and add nothing."""
    counts = np.asarray(counts)
    px = tile_pixels(cam, tile)
    rgb, lin = np.zeros((len(px), 3), np.uint8), np.full((len(px), 3), np.nan)
    segs, rc = 0, abi.RT_OK
    for n in np.unique(counts[counts > 0]):
        sel = np.flatnonzero(counts == n)
        r, l, s, c = oracle_class(key, flat, cam, depth, int(n), flags, px[sel], seed)
        rgb[sel], lin[sel] = r, l
        segs += s
        rc = max(rc, c)
    return rgb, lin, segs, rc


def open_session(renderer, flat, cam, cap, flags, depth=DEPTH, tile=None, seed=SEED):
    renderer.seed, renderer.flags = seed, flags
    return renderer.begin_progressive(depth, cap, flat, cam, tile_range=tile)


def check_map(key, got, counts, traced, segs_so_far, flat, cam, flags, depth=DEPTH, tile=None, items=True):
    """One image (rgb, lin, st, rc) of a session at per-pixel counts against the oracle, and the step's stats:
    `traced` samples since the last collect, segs_so_far the segments of every collect up to this one."""
    rgb, lin, st, rc = got
    rgb_o, lin_o, segs_o, rc_o = oracle_map(key, flat, cam, depth, counts, flags, tile)
    bad = np.argwhere(lin != lin_o)
    assert bad.size == 0, f"{key}: {len(bad)} channels differ from the oracle; first pixel {bad[0][0]} at " \
                          f"{counts[bad[0][0]]} spp: {lin[bad[0][0]]} / {lin_o[bad[0][0]]}"
    np.testing.assert_array_equal(rgb, rgb_o)
    assert rc == rc_o, (key, rc, rc_o)
    assert segs_so_far == segs_o, (key, segs_so_far, segs_o)
    assert st.samples == traced and st.pixels == len(counts), (key, st.samples, traced, st.pixels)
    assert abi.RT_KERNEL_SPLIT(st.kernel_id), hex(st.kernel_id)
    assert bool(abi.RT_KERNEL_ITEMS(st.kernel_id)) == items, hex(st.kernel_id)
    k = abi.kernel_info(st.kernel_id)
    assert k["T"] == ("float" if flags & F32 else "double") and k["W"] == (5 if flags & F32 else 4)
    return st


def plan(lib, done, target, waves):
    """rt_progressive_map_plan: (S, items [n, 3] of pixel, first, end)."""
    done, target = np.ascontiguousarray(done, np.uint32), np.ascontiguousarray(target, np.uint32)
    s, n = ctypes.c_uint32(), ctypes.c_uint64()
    args = (len(done), done.ctypes.data_as(U32P), target.ctypes.data_as(U32P), waves, ctypes.byref(s), ctypes.byref(n))
    assert lib.rt_progressive_map_plan(*args, None, 0) == abi.RT_OK
    items = np.zeros((n.value, 4), np.uint32)
    assert lib.rt_progressive_map_plan(*args, items.ctypes.data_as(U32P), n.value) == abi.RT_OK
    return s.value, items[:, :3]


# ---- 1, 2. counts from zero, then steps ----
TARGETS_1 = np.array([1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300, 512], np.uint32)
# deltas: 0, +1, 0, across a chunk of 4, across 64, 0, across the 128 grain (far), across it (near), 0, off-grain to
# off-grain, to capacity, 0 at capacity
TARGETS_2 = np.array([1, 4, 4, 10, 70, 64, 200, 129, 128, 131, 512, 512], np.uint32)


def counts_from_zero(renderer, session, flags, flat, cam):
    got = session.extend_map(TARGETS_1, want_linear=True)
    np.testing.assert_array_equal(session.counts, TARGETS_1)
    assert session.done == 1
    check_map(("zero", flags), got, TARGETS_1, int(TARGETS_1.sum()), got[2].ray_segments, flat, cam, flags)
    return got[2].ray_segments


@pytest.mark.parametrize("flags", [0, F32])
def test_counts_from_zero(renderer, scene_100, flags):
    """4x3, capacity 512, one map from zero: counts of 1, around a chunk of 4, around a 64-sample camera batch,
    around the 128 grain, off the grain, and the capacity."""
    cam = cam_for(4, 3)
    with open_session(renderer, scene_100, cam, 512, flags) as s:
        counts_from_zero(renderer, s, flags, scene_100, cam)


@pytest.mark.parametrize("flags", [0, F32])
def test_steps(renderer, scene_100, flags):
    """From test_counts_from_zero's state a second map with every kind of delta, then the refusal of a uniform
    extend below the largest count, then extend(512): the whole frame equals rt_render_async at 512."""
    cam, lib = cam_for(4, 3), renderer.lib
    with open_session(renderer, scene_100, cam, 512, flags) as s:
        segs = counts_from_zero(renderer, s, flags, scene_100, cam)
        got = s.extend_map(TARGETS_2, want_linear=True)
        np.testing.assert_array_equal(s.counts, TARGETS_2)
        segs += got[2].ray_segments
        check_map(("zero", flags), got, TARGETS_2, int((TARGETS_2 - TARGETS_1).sum()), segs, scene_100, cam, flags)
        assert lib.rt_progressive_extend_async(renderer.ctx, 511, None, None, None) == abi.RT_ERR_INVALID
        assert b"rt_progressive_extend_async" in lib.rt_last_error()
        np.testing.assert_array_equal(s.counts, TARGETS_2)
        got = s.extend(512, want_linear=True)
        assert s.done == 512 and (s.counts == 512).all()
        segs += got[2].ray_segments
        full = np.full(12, 512, np.uint32)
        check_map(("zero", flags), got, full, int((full - TARGETS_2).sum()), segs, scene_100, cam, flags)
        renderer.seed, renderer.flags = SEED, flags
        rgb_u, lin_u, st_u, rc_u = renderer.render_flat(DEPTH, 512, scene_100, cam, want_linear=True)
        np.testing.assert_array_equal(got[1], lin_u)
        np.testing.assert_array_equal(got[0], rgb_u)
        assert got[3] == rc_u and segs == st_u.ray_segments and got[2].bounce_iters == st_u.bounce_iters


# ---- 3. several items per pixel, unequal starts ----
def test_several_items_per_pixel(renderer, lib, scene_100):
    """A 2x1 tile at capacity 4096: [4096, 130], then [4096, 2500].  On an MI355X both maps are dealt into items
    of 128 samples, several per pixel, the second from an off-grain start of one pixel only."""
    cam, tile = cam_for(16, 9), abi.RtTileRange(3, 1, 1, 5, 2)
    t1, t2 = np.array([4096, 130], np.uint32), np.array([4096, 2500], np.uint32)
    s1, items1 = plan(lib, [0, 0], t1, MI355X_WAVES[F32])
    s2, items2 = plan(lib, t1, t2, MI355X_WAVES[F32])
    assert s1 % 128 == 0 and (items1[:, 0] == 0).sum() > 1 and (items1[:, 0] == 1).sum() > 1
    assert s2 % 128 == 0 and (items2[:, 0] == 1).sum() > 1 and not (items2[:, 0] == 0).any()
    assert items2[0].tolist() == [1, 130, 256]
    with open_session(renderer, scene_100, cam, 4096, F32, tile=tile) as s:
        got = s.extend_map(t1, want_linear=True)
        segs = got[2].ray_segments
        check_map(("tile2",), got, t1, int(t1.sum()), segs, scene_100, cam, F32, tile=tile)
        got = s.extend_map(t2, want_linear=True)
        segs += got[2].ray_segments
        check_map(("tile2",), got, t2, 2370, segs, scene_100, cam, F32, tile=tile)


# ---- 4. snapshots at earlier counts ----
def test_snapshots_at_earlier_counts(renderer, scene_100):
    cam, flags = cam_for(4, 3), F32
    earlier = np.array([1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 63, 64], np.uint32)
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        s.extend(64, image=False)
        got = s.snapshot(earlier, want_linear=True)
        rgb_o, lin_o, _, rc_o = oracle_map(("zero", flags), scene_100, cam, DEPTH, earlier, flags)
        np.testing.assert_array_equal(got[1], lin_o)
        np.testing.assert_array_equal(got[0], rgb_o)
        assert got[3] == rc_o
        assert (got[2].samples, got[2].ray_segments, got[2].pixels) == (0, 0, 12) and got[2].bounce_iters > 0
        assert abi.RT_KERNEL_SPLIT(got[2].kernel_id) and not abi.RT_KERNEL_ITEMS(got[2].kernel_id)
        assert (s.counts == 64).all()                       # a snapshot moves no count
        got = s.snapshot(None, want_linear=True)
        rgb_o, lin_o, _, rc_o = oracle_map(("zero", flags), scene_100, cam, DEPTH, np.full(12, 64), flags)
        np.testing.assert_array_equal(got[1], lin_o)
        np.testing.assert_array_equal(got[0], rgb_o)
        assert got[2].samples == 0 and got[3] == rc_o
        for bad in (0, 65):
            c = earlier.copy()
            c[7] = bad
            with pytest.raises(rt.RtError) as e:
                s.snapshot(c)
            assert e.value.code == abi.RT_ERR_INVALID and "rt_progressive_snapshot_map_async" in str(e.value)


# ---- 5. the error estimate ----
def oracle_error(key, flat, cam, counts, flags):
    counts = np.asarray(counts)
    full = oracle_map(key, flat, cam, DEPTH, counts, flags)[1]
    half = oracle_map(key, flat, cam, DEPTH, counts // 2, flags)[1]
    err = np.abs(full - half).max(axis=1)
    err[counts < 2] = np.inf
    return err


def mixed_counts(values, n):
    """n counts cycling through `values` with a stride that is odd against the row length, so every value lands
    in sky and sphere pixels alike."""
    return np.array([values[(7 * i) % len(values)] for i in range(n)], np.uint32)


@pytest.mark.parametrize("flags", [0, F32])
def test_error_estimate(renderer, scene_100, flags):
    """16x9.  A session at 8 spp everywhere: the estimate is |lin(8) - lin(4)|; the same session after a map
    mixing 8, 16 and 33: |lin(n) - lin(n // 2)| per pixel.  Counts only grow, so the count-1 pixels are in a second
    session, whose first map mixes 1, 8, 16 and 33: those pixels read inf.  Equality is ==, not a tolerance."""
    cam, key, n = cam_for(16, 9), ("err", flags), 16 * 9
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        s.extend(8, image=False)
        err, st = s.error(stats=True)
        assert err.dtype == np.float64 and err.shape == (n,)
        np.testing.assert_array_equal(err, oracle_error(key, scene_100, cam, np.full(n, 8), flags))
        assert (st.samples, st.ray_segments, st.pixels) == (0, 0, n) and st.bounce_iters > 0
        counts = mixed_counts([8, 16, 33], n)
        s.extend_map(counts, image=False)
        np.testing.assert_array_equal(s.error(), oracle_error(key, scene_100, cam, counts, flags))
    with open_session(renderer, scene_100, cam, 64, flags) as s:
        counts = mixed_counts([1, 8, 16, 33], n)
        s.extend_map(counts, image=False)
        err = s.error()
        assert np.isposinf(err[counts == 1]).all() and np.isfinite(err[counts > 1]).all()
        np.testing.assert_array_equal(err, oracle_error(key, scene_100, cam, counts, flags))
        np.testing.assert_array_equal(s.counts, counts)     # the estimate moves no count


# ---- 6. a whole adaptive run ----
def replay(key, flat, cam, flags, spp_min, spp_max, tolerance=None):
    """GpuRenderer.adaptive's policy with the oracle: (counts, tolerance, steps).  tolerance None: the median of
    the first error."""
    n = cam.image_width * cam.image_height
    counts, steps = np.full(n, spp_min, np.uint32), 0
    while True:
        err = oracle_error(key, flat, cam, counts, flags)
        if tolerance is None:
            tolerance = float(np.median(err))
            assert not (err == tolerance).any()             # no pixel sits on the threshold
        active = (err > tolerance) & (counts < spp_max)
        if not active.any():
            return counts, tolerance, steps
        counts[active] = np.minimum(2 * counts[active], spp_max)
        steps += 1


@pytest.mark.parametrize("flags", [0, F32])
def test_adaptive_run(renderer, scene_100, flags):
    """16x9, 8 to 64 spp, the tolerance at the median of the first error: the run's count map equals the
    oracle's replay of the policy, the image is the oracle's per class, and the samples traced are the counts'."""
    cam, key = cam_for(16, 9), ("err", flags)
    want, tol, steps = replay(key, scene_100, cam, flags, 8, 64)
    assert len(np.unique(want)) >= 2 and steps >= 1
    renderer.seed, renderer.flags = SEED, flags
    img, counts, stat = renderer.adaptive(DEPTH, 8, 64, tol, scene_100, cam)
    assert img.shape == (9, 16, 3) and img.dtype == np.uint8 and counts.shape == (9, 16) and counts.dtype == np.uint32
    np.testing.assert_array_equal(counts.reshape(-1), want)
    rgb_o, _, segs_o, rc_o = oracle_map(key, scene_100, cam, DEPTH, want, flags)
    assert rc_o == abi.RT_OK
    np.testing.assert_array_equal(img.reshape(-1, 3), rgb_o)
    assert stat.samples == int(counts.sum()) and stat.ray_segments == segs_o


# ---- 7. record formats and kernels ----
SMALL = np.array([1, 5, 64, 33, 2, 17, 64, 40, 3, 8, 63, 16], np.uint32)


def one_map(renderer, key, flat, cam, cap, counts, flags, depth=DEPTH, tile=None):
    with open_session(renderer, flat, cam, cap, flags, depth=depth, tile=tile) as s:
        got = s.extend_map(counts, want_linear=True)
        return check_map(key, got, counts, int(np.asarray(counts).sum()), got[2].ray_segments, flat, cam, flags,
                         depth=depth, tile=tile)


@pytest.mark.parametrize("flags", [0, F32])
def test_defocus_camera(renderer, scene_100, flags):
    """The kernels without camera batches."""
    st = one_map(renderer, ("defocus", flags), scene_100, cam_for(4, 3, defocus_angle=2.0), 64, SMALL, flags)
    assert not abi.kernel_info(st.kernel_id)["camq"]


def test_row_strided_tile(renderer, scene_100):
    tile = abi.RtTileRange(1, 3, 3, 5, 4)   # rows 1, 4, 7 of 9; columns 5..8 of 16
    one_map(renderer, ("strided",), scene_100, cam_for(16, 9), 64, SMALL, F32, tile=tile)


def test_wide_termination_bounces(renderer, scene_100):
    """depth 300 > 254: u32 e in the session's regions."""
    one_map(renderer, ("e32",), scene_100, cam_for(4, 3), 64, SMALL, 0, depth=300)


def test_config_e_scene(renderer):
    """Config E's 10 000 spheres: the mega item-table kernel."""
    st = one_map(renderer, ("E",), rt.scenes.config_scene("E").flatten(), cam_for(4, 3), 64, SMALL, F32)
    assert abi.kernel_info(st.kernel_id)["mega"]


def test_position_map_widths_by_class(renderer, scene_100):
    """A 2x1 tile at capacity 33 000 with counts [33000, 100]: a u32 position map in one class's reduction, a u16
    map in the other's, out of regions of one layout."""
    tile = abi.RtTileRange(4, 1, 1, 7, 2)
    one_map(renderer, ("wide",), scene_100, cam_for(16, 9), 33000, np.array([33000, 100], np.uint32), F32, tile=tile)


# ---- 8. interleaving ----
def test_interleaving(renderer, scene_100):
    """An rt_render_async of another camera and seed between two map extends on the same context, without a
    collect in between: each of the three images is what it is alone."""
    cams = [cam_for(4, 3), cam_for(4, 3, center=(13.0, 3.0, -8.0))]
    lib, ctx, npx = renderer.lib, renderer.ctx, 12
    renderer.seed, renderer.flags = 22, F32
    other = renderer.render_flat(DEPTH, 96, scene_100, cams[1], want_linear=True)[1]
    bufs = [ctypes.c_void_p() for _ in range(3)]
    for b in bufs:
        abi.check(lib, lib.rt_device_alloc(ctx, npx * 24, ctypes.byref(b)))
    tr = abi.RtTileRange(0, 1, 3, 0, 4)
    try:
        abi.check(lib, lib.rt_progressive_begin(ctx, ctypes.byref(cams[0]), DEPTH, 512, SEED, F32, ctypes.byref(tr), 0))
        try:
            abi.check(lib, lib.rt_progressive_extend_map_async(ctx, TARGETS_1.ctypes.data_as(U32P), None, bufs[0], None))
            abi.check(lib, lib.rt_render_async(ctx, ctypes.byref(cams[1]), DEPTH, 96, 22, F32, ctypes.byref(tr), None,
                                               bufs[1], None))
            abi.check(lib, lib.rt_progressive_extend_map_async(ctx, TARGETS_2.ctypes.data_as(U32P), None, bufs[2], None))
            st = abi.RtStats()
            # the collect's code is the worst of the three (a pixel at 1 spp may be RT_ERR_RANGE, as in the oracle)
            abi.check(lib, lib.rt_context_collect(ctx, None, ctypes.byref(st)), allow=(abi.RT_ERR_RANGE,))
            assert st.samples == int(TARGETS_2.sum()) + npx * 96 and st.pixels == 3 * npx
            out = [np.empty((npx, 3)) for _ in bufs]
            for o, b in zip(out, bufs):
                abi.check(lib, lib.rt_memcpy_d2h(ctx, o.ctypes.data, b, npx * 24))
        finally:
            abi.check(lib, lib.rt_progressive_end(ctx))
    finally:
        for b in bufs:
            lib.rt_device_free(ctx, b)
    np.testing.assert_array_equal(out[0], oracle_map(("zero", F32), scene_100, cams[0], DEPTH, TARGETS_1, F32)[1])
    np.testing.assert_array_equal(out[2], oracle_map(("zero", F32), scene_100, cams[0], DEPTH, TARGETS_2, F32)[1])
    np.testing.assert_array_equal(out[1], other)


# ---- 9. refusals ----
def test_refusals(renderer, scene_100):
    lib, ctx = renderer.lib, renderer.ctx
    renderer.set_scene(scene_100)
    cam, tr, n = cam_for(20, 16), abi.RtTileRange(0, 1, 16, 0, 20), 320
    buf = ctypes.c_void_p()
    abi.check(lib, lib.rt_device_alloc(ctx, n * 24, ctypes.byref(buf)))

    def arr(v):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint32), (n,)))
        return a, a.ctypes.data_as(U32P)

    def extend_map(v, out=None):
        a, p = arr(v)
        return lib.rt_progressive_extend_map_async(ctx, p, None, out, None)

    def snapshot(v, out=buf):
        a, p = arr(v)
        return lib.rt_progressive_snapshot_map_async(ctx, p, None, out, None)

    def refused(rc, code, who):
        assert rc == code, (rc, lib.rt_last_error())
        assert who in lib.rt_last_error(), lib.rt_last_error()

    def collect():
        st = abi.RtStats()
        assert lib.rt_context_collect(ctx, None, ctypes.byref(st)) in (abi.RT_OK, abi.RT_ERR_RANGE)
        return st

    counts_out = np.zeros(n, np.uint32)
    try:
        # no session open
        refused(extend_map(4), abi.RT_ERR_INVALID, b"rt_progressive_extend_map_async")
        refused(snapshot(4), abi.RT_ERR_INVALID, b"rt_progressive_snapshot_map_async")
        refused(lib.rt_progressive_counts(ctx, counts_out.ctypes.data_as(U32P)), abi.RT_ERR_INVALID, b"rt_progressive_counts")
        refused(lib.rt_progressive_error_async(ctx, buf, None), abi.RT_ERR_INVALID, b"rt_progressive_error_async")
        abi.check(lib, lib.rt_progressive_begin(ctx, ctypes.byref(cam), DEPTH, 300, SEED, F32, ctypes.byref(tr), 0))
        try:
            refused(lib.rt_progressive_extend_map_async(ctx, None, None, buf, None), abi.RT_ERR_INVALID,
                    b"rt_progressive_extend_map_async")
            refused(lib.rt_progressive_counts(ctx, None), abi.RT_ERR_INVALID, b"rt_progressive_counts")
            refused(lib.rt_progressive_error_async(ctx, None, None), abi.RT_ERR_INVALID, b"rt_progressive_error_async")
            refused(snapshot(1), abi.RT_ERR_INVALID, b"rt_progressive_snapshot_map_async")      # above done_p = 0
            base = np.full(n, 4, np.uint32)
            base[5] = 0
            refused(extend_map(base, buf), abi.RT_ERR_INVALID, b"rt_progressive_extend_map_async")   # 0 with an output
            assert extend_map(base) == abi.RT_OK                                                # trace only: untouched
            assert collect().samples == 4 * (n - 1)
            assert lib.rt_progressive_counts(ctx, counts_out.ctypes.data_as(U32P)) == abi.RT_OK
            np.testing.assert_array_equal(counts_out, base)
            low, high = base.copy(), base.copy()
            low[9], high[9] = 3, 301
            refused(extend_map(low), abi.RT_ERR_INVALID, b"rt_progressive_extend_map_async")    # below done_p
            refused(extend_map(high), abi.RT_ERR_INVALID, b"rt_progressive_extend_map_async")   # above the capacity
            refused(snapshot(base), abi.RT_ERR_INVALID, b"rt_progressive_snapshot_map_async")   # a count of 0
            refused(snapshot(np.maximum(base, 1), None), abi.RT_ERR_INVALID, b"rt_progressive_snapshot_map_async")
            # 300 distinct counts: unsupported with an output, accepted trace only
            many = (np.arange(n, dtype=np.uint32) % 300) + 4
            many[many > 300] = 300
            assert len(np.unique(many)) > 256
            refused(extend_map(many, buf), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_extend_map_async")
            assert lib.rt_progressive_counts(ctx, counts_out.ctypes.data_as(U32P)) == abi.RT_OK
            np.testing.assert_array_equal(counts_out, base)                                     # a refusal moves nothing
            assert extend_map(many) == abi.RT_OK
            st = collect()
            assert st.samples == int((many - base).sum()) and abi.RT_KERNEL_ITEMS(st.kernel_id)
            refused(snapshot(many), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_snapshot_map_async")
            refused(lib.rt_progressive_error_async(ctx, buf, None), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_error_async")
            assert snapshot(4) == abi.RT_OK and collect().samples == 0
        finally:
            assert lib.rt_progressive_end(ctx) == abi.RT_OK
        st = collect()
        assert st.samples == 0 and st.kernel_id == 0
    finally:
        lib.rt_device_free(ctx, buf)


def test_session_argument_checks(renderer, scene_100):
    """ProgressiveSession refuses a map of the wrong length or type before any GPU call."""
    with open_session(renderer, scene_100, cam_for(4, 3), 16, F32) as s:
        for bad in (np.zeros(11, np.uint32), np.zeros(12, np.float64), np.full(12, -1), np.zeros((3, 4), np.uint32)):
            with pytest.raises(ValueError):
                s.extend_map(bad)
            with pytest.raises(ValueError):
                s.snapshot(bad)
        assert (s.counts == 0).all() and s.done == 0


# ---- 10. CLI ----
def test_cli_adaptive(tmp_path, lib):
    """rt-render --adaptive to a .ppm: its pixel bytes equal GpuRenderer.adaptive's image, and --count-map is
    255 * counts // spp as grey RGB8."""
    cli = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-ray-tracing_amd", "bin", "rt-render")
    scene = rt.scenes.three_spheres()
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(scene))
    tol = 0.02
    args = [cli, "--width", "16", "--height", "9", "--spp", "64", "--bounces", "8", "--f32", "--adaptive", repr(tol),
            "--spp-min", "8", "--count-map", "counts.ppm", "--out", "o.ppm"]
    r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = rt.GpuRenderer(lib=lib, precision="f32")
    try:
        img, counts, stat = g.adaptive(8, 8, 64, tol, scene, rt.Camera(16, 9, **rt.MAIN_CAMERA))
    finally:
        g.close()
    assert len(np.unique(counts)) >= 2
    raw = (tmp_path / "o.ppm").read_bytes()
    assert raw.startswith(b"P6")
    np.testing.assert_array_equal(np.frombuffer(raw[-16 * 9 * 3:], np.uint8).reshape(9, 16, 3), img)
    raw = (tmp_path / "counts.ppm").read_bytes()
    grey = (255 * counts.astype(np.uint64) // 64).astype(np.uint8)
    np.testing.assert_array_equal(np.frombuffer(raw[-16 * 9 * 3:], np.uint8).reshape(9, 16, 3),
                                  np.repeat(grey[:, :, None], 3, axis=2))
    steps = [ln for ln in r.stdout.splitlines() if ln.startswith("Adaptive: ")]
    assert len(steps) >= 2 and f"{stat.samples} samples" in steps[-1] and "active" in steps[0]
    for flag in (["--root2"], ["--mode", "scalar"], ["--block-size", "64"], ["--progressive", "16"]):
        bad = subprocess.run(args + flag, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--adaptive" in bad.stderr, (flag, bad.stderr)
