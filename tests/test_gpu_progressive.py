"""Progressive sessions (rt_progressive_begin / _extend_async / _end: trace_paths_window over the sample
window of every pixel, then finish_window over the prefix) against the CPU oracle and against rt_render_async.

Bar: 0 ulp, at every snapshot.  After extend(n) the linear image, the RGB8 bytes and the return code equal
oracle_render's at spp = n, and the ray_segments summed over the session's collects equal the oracle's segments
at n.  Where it is cheap the snapshot is also compared with rt_render_async at n, bounce_iters included.  The
shapes are a few pixels by at most a few thousand samples: the smallest at which each part can go wrong
(windows that start inside a chunk, a camera batch or off the 128 grain, capacity above the count, every
record format, both camera paths, the mega kernels, K > 64, several items per pixel).
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
EMPTY = lambda: rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32),   # noqa: E731
                             [rt.Lambertian((0.5, 0.5, 0.5))])


def cam_for(w, h, **kw):
    return rt.camera_new_py(w, h, **dict(rt.MAIN_CAMERA, **kw))


@pytest.fixture(scope="module")
def scene_100():
    return rt.scenes.random_spheres(100).flatten()


def tile_pixels(cam, tile):
    """Global pixel indices of a tile range, in the output's order."""
    rows = tile.row_begin + np.arange(tile.row_count, dtype=np.int64) * tile.row_step
    cols = tile.col_begin + np.arange(tile.col_count, dtype=np.int64)
    return (rows[:, None] * cam.image_width + cols[None, :]).reshape(-1).astype(np.uint32)


_refs = {}


def reference(key, flat, cam, depth, spp, flags, pixels=None, seed=SEED):
    """oracle_render at one sample count, computed once per key and left unchanged."""
    key = ("oracle",) + key + (spp,)
    if key not in _refs:
        r = oracle_render(flat, cam, depth, spp, seed, 0, pixels=pixels, precision="f32" if flags & F32 else "f64")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def unsplit(renderer, key, flat, cam, depth, spp, flags, tile=None, seed=SEED):
    """rt_render_async at one sample count, once per key."""
    key = ("async",) + key + (spp,)
    if key not in _refs:
        renderer.seed, renderer.flags = seed, flags
        _refs[key] = renderer.render_flat(depth, spp, flat, cam, tile_range=tile, want_linear=True)
    return _refs[key]


def open_session(renderer, flat, cam, depth, cap, flags, tile=None, seed=SEED, max_bytes=0):
    renderer.seed, renderer.flags = seed, flags
    return renderer.begin_progressive(depth, cap, flat, cam, tile_range=tile, max_bytes=max_bytes)


def check_snapshot(key, got, n, new_samples, segs_so_far, npx, flat, cam, depth, flags, px=None, renderer=None, tile=None,
                   rc_want=None):
    """One snapshot (rgb, lin, st, rc) at n samples: the oracle at spp = n, the stats of the step, and, with a
    renderer, rt_render_async at n."""
    rgb, lin, st, rc = got
    rgb_o, lin_o, segs_o, rc_o = reference(key, flat, cam, depth, n, flags, pixels=px)
    bad = np.argwhere(lin != lin_o)
    assert bad.size == 0, f"{key} at {n} spp: {len(bad)} channels differ from the oracle; first pixel {bad[0][0]}: " \
                          f"{lin[bad[0][0]]} / {lin_o[bad[0][0]]}"
    np.testing.assert_array_equal(rgb, rgb_o)
    assert rc == rc_o and (rc_want is None or rc == rc_want), (key, n, rc, rc_o)
    assert segs_so_far == segs_o, (key, n)
    assert st.samples == npx * new_samples and st.pixels == npx, (key, n, st.samples, st.pixels)
    assert abi.RT_KERNEL_SPLIT(st.kernel_id), hex(st.kernel_id)
    k = abi.kernel_info(st.kernel_id)
    assert k["T"] == ("float" if flags & F32 else "double") and k["W"] == (5 if flags & F32 else 4)
    assert st.kernel_wg_per_cu >= k["W"] and st.direct_sky_samples == 0
    if renderer is not None:
        rgb_u, lin_u, st_u, rc_u = unsplit(renderer, key, flat, cam, depth, n, flags, tile)
        np.testing.assert_array_equal(lin, lin_u)
        np.testing.assert_array_equal(rgb, rgb_u)
        assert rc == rc_u
        assert st.bounce_iters == st_u.bounce_iters and segs_so_far == st_u.ray_segments, (key, n)
    return st


def run_schedule(renderer, key, flat, cam, depth, cap, schedule, flags, tile=None, against_async=True, rc_want=None):
    """A session of capacity cap extended through schedule, every step checked; returns the steps' stats.
    The rt_render_async renders it is compared with run on the same context while the session is open."""
    px = tile_pixels(cam, tile) if tile is not None else None
    npx = tile.row_count * tile.col_count if tile is not None else cam.image_width * cam.image_height
    stats, segs, prev = [], 0, 0
    with open_session(renderer, flat, cam, depth, cap, flags, tile) as session:
        for n in schedule:
            got = session.extend(n, want_linear=True)
            assert session.done == n
            segs += got[2].ray_segments
            stats.append(check_snapshot(key, got, n, n - prev, segs, npx, flat, cam, depth, flags, px,
                                        renderer if against_async else None, tile, rc_want))
            prev = n
    return stats


# ---- 1. window edges ----
@pytest.mark.parametrize("flags", [0, F32])
def test_window_edges(renderer, scene_100, flags):
    """4x3, capacity 512: windows that start inside a chunk of 4 (6 -> 7), inside a 64-sample camera batch
    (7 -> 100, 100 -> 128) and off the 128 grain (129 -> 512), both parities of (C - 1) % 2, a partial last
    chunk (6, 7, 129), one sample, and count == capacity."""
    run_schedule(renderer, ("edges", flags), scene_100, cam_for(4, 3), 50, 512, [1, 6, 7, 100, 128, 129, 512], flags)


# ---- 2. capacity != count ----
@pytest.mark.parametrize("flags", [0, F32])
def test_capacity_above_count(renderer, scene_100, flags):
    """Regions laid out for 4096 samples reduced at 100 and 512: strides from P_cap, reduction from P.  The
    same references as test_window_edges (same key), so a session at capacity 512 gives the same images."""
    run_schedule(renderer, ("edges", flags), scene_100, cam_for(4, 3), 50, 4096, [100, 512], flags)
    run_schedule(renderer, ("edges", flags), scene_100, cam_for(4, 3), 50, 512, [100, 512], flags)


# ---- 3. snapshot and trace-only ----
@pytest.mark.parametrize("flags", [0, F32])
def test_snapshot_and_trace_only(renderer, scene_100, flags):
    cam, key, npx = cam_for(4, 3), ("edges", flags), 12
    _, _, segs64, _ = reference(key, scene_100, cam, 50, 64, flags)
    with open_session(renderer, scene_100, cam, 50, 512, flags) as s:
        st = s.extend(64, image=False)                       # traces, reduces nothing
        assert (st.samples, st.pixels, st.ray_segments, st.bounce_iters) == (npx * 64, npx, segs64, 0)
        assert abi.RT_KERNEL_SPLIT(st.kernel_id)
        a = s.extend(64, want_linear=True)                   # a snapshot: the reduction only
        assert (a[2].samples, a[2].pixels, a[2].ray_segments) == (0, npx, 0) and a[2].bounce_iters > 0
        b = s.extend(64, want_linear=True)
        assert (b[2].samples, b[2].ray_segments, b[2].bounce_iters) == (0, 0, a[2].bounce_iters)
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[0], b[0])
        rgb_o, lin_o, _, rc_o = reference(key, scene_100, cam, 50, 64, flags)
        np.testing.assert_array_equal(a[1], lin_o)
        np.testing.assert_array_equal(a[0], rgb_o)
        assert a[3] == b[3] == rc_o
        st = s.extend(64, image=False)                       # nothing to do: nothing enqueued
        assert (st.samples, st.pixels, st.kernel_id, st.ray_segments) == (0, 0, 0, 0)
        st200 = s.extend(200, image=False)
        assert st200.samples == npx * 136 and s.done == 200
        got = s.extend(256, want_linear=True)
        check_snapshot(key, got, 256, 56, segs64 + st200.ray_segments + got[2].ray_segments, npx, scene_100, cam, 50, flags,
                       renderer=renderer)


# ---- 4. position-map widths ----
@pytest.mark.parametrize("cap,schedule,flags", [(70001, [32761, 32765, 70001], F32), (32765, [32761, 32765], 0)])
def test_position_map_widths(renderer, scene_100, cap, schedule, flags):
    """P = 32764 (the last u16 map) and 32768 (the first u32 map) in regions laid out for more: the map's
    width follows the snapshot's count; then the wide capacity itself."""
    run_schedule(renderer, ("wide", flags), scene_100, cam_for(2, 1), 50, cap, schedule, flags)


# ---- 5. u32 termination bounces ----
def test_wide_termination_bounces(renderer, scene_100):
    """depth 300 > 254: u32 e in the session's regions."""
    run_schedule(renderer, ("e32",), scene_100, cam_for(16, 9), 300, 256, [128, 256], 0)


# ---- 6. depth 0, 1, 2 ----
@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("flags", [0, F32])
def test_depth_edges(renderer, scene_100, depth, flags):
    run_schedule(renderer, ("depth", depth, flags), scene_100, cam_for(8, 5), depth, 256, [64, 256], flags)


# ---- 7. defocus camera ----
@pytest.mark.parametrize("flags", [0, F32])
def test_defocus_camera(renderer, scene_100, flags):
    """The kernels without camera batches (every primary ray has its own origin)."""
    sts = run_schedule(renderer, ("defocus", flags), scene_100, cam_for(8, 5, defocus_angle=2.0), 50, 256, [100, 256], flags)
    assert not abi.kernel_info(sts[-1].kernel_id)["camq"]


# ---- 8. sky only ----
@pytest.mark.parametrize("flags", [0, F32])
def test_sky_only(renderer, scene_100, flags):
    """The empty scene, and a camera that sees no sphere: every sample writes e = 0 and the snapshot is the
    sky-only reduction over a prefix."""
    run_schedule(renderer, ("empty", flags), EMPTY(), cam_for(8, 5), 50, 512, [128, 512], flags)
    up = cam_for(8, 5, center=(0.0, 30.0, 0.0), look_at=(3.0, 60.0, 1.0))
    sts = run_schedule(renderer, ("sky", flags), scene_100, up, 50, 512, [128, 512], flags)
    assert sum(st.ray_segments for st in sts) == 8 * 5 * 512   # one segment per sample: every primary ray escapes


# ---- 9. mega kernels ----
def test_config_e_scene(renderer):
    """Config E's 10 000 spheres: the mega kernels."""
    flat = rt.scenes.config_scene("E").flatten()
    sts = run_schedule(renderer, ("E",), flat, cam_for(4, 3), 50, 2048, [256, 2048], F32)
    assert all(abi.kernel_info(st.kernel_id)["mega"] for st in sts)


# ---- 10. K > 64 ----
def cage():
    """Six large fuzzy-mirror spheres that overlap around the camera (their surfaces 3 units away on every
    side).  A ray bounces between them until a fuzzed reflection leaves through a seam: the mean path is ~132
    bounces of 200, so short paths and paths that last all 200 bounces mix in every pixel and every pixel has
    K > 64 (finish_pixel's per-bounce replay)."""
    c = np.array(rt.MAIN_CAMERA["center"])
    off = [(103.0, 0, 0), (-103.0, 0, 0), (0, 0, 103.0), (0, 0, -103.0), (0, -103.0, 0), (0, 103.0, 0)]
    return rt.FlatScene(np.array([c + np.array(o) for o in off]), np.full(6, 100.0), np.zeros(6, np.uint32),
                        [rt.Metal((0.97, 0.95, 0.9), 0.3)])


@pytest.mark.parametrize("flags", [0, F32])
def test_long_paths(renderer, flags):
    sts = run_schedule(renderer, ("cage", flags), cage(), cam_for(16, 9), 200, 24, [8, 24], flags)
    assert all(st.bounce_iters > 64 * 16 * 9 for st in sts)


# ---- 11. strided tile ----
@pytest.mark.parametrize("flags", [0, F32])
def test_row_strided_tile(renderer, scene_100, flags):
    tile = abi.RtTileRange(1, 3, 18, 5, 80)   # rows 1, 4, ..., 52 of 54; columns 5..84 of 96
    run_schedule(renderer, ("strided", flags), scene_100, cam_for(96, 54), 50, 256, [128, 256], flags, tile=tile)


# ---- 12. many items ----
def test_many_items(renderer, lib, scene_100):
    """64x36 at capacity 4096: the second extend's window of 3584 samples is dealt into several items per
    pixel (the plan of rt_split_plan over the window on an MI355X: 256 CUs x 4 SIMDs x 5 waves)."""
    s, n = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.rt_split_plan(64 * 36, 4096 - 512, 256 * 4 * 5, ctypes.byref(s), ctypes.byref(n)) == 0
    assert n.value > 64 * 36 and s.value % 128 == 0 and s.value < 4096 - 512
    run_schedule(renderer, ("thumb",), scene_100, cam_for(64, 36), 50, 4096, [512, 4096], F32, against_async=False)


# ---- 13. interleaving ----
class Raw:
    """The async API without a collect in between."""

    def __init__(self, renderer, flat, npx):
        self.lib, self.ctx, self.npx = renderer.lib, renderer.ctx, npx
        renderer.set_scene(flat)
        self.bufs = []

    def buf(self):
        b = ctypes.c_void_p()
        abi.check(self.lib, self.lib.rt_device_alloc(self.ctx, self.npx * 24, ctypes.byref(b)))
        self.bufs.append(b)
        return b

    def render(self, cam, depth, spp, seed, flags, stream, S):
        b = self.buf()
        tr = abi.RtTileRange(0, 1, cam.image_height, 0, cam.image_width)
        if S is None:
            rc = self.lib.rt_render_async(self.ctx, ctypes.byref(cam), depth, spp, seed, flags, ctypes.byref(tr), None, b, stream)
        else:
            rc = self.lib.rt_render_split_async(self.ctx, ctypes.byref(cam), depth, spp, seed, flags, ctypes.byref(tr),
                                                None, b, stream, S)
        abi.check(self.lib, rc)
        return b

    def extend(self, n, stream, image=True):
        b = self.buf() if image else None
        abi.check(self.lib, self.lib.rt_progressive_extend_async(self.ctx, n, None, b, stream))
        return b

    def collect(self, stream):
        st = abi.RtStats()
        abi.check(self.lib, self.lib.rt_context_collect(self.ctx, stream, ctypes.byref(st)))
        return st

    def read(self, b):
        out = np.empty((self.npx, 3), dtype=np.float64)
        abi.check(self.lib, self.lib.rt_memcpy_d2h(self.ctx, out.ctypes.data, b, self.npx * 24))
        return out

    def close(self):
        for b in self.bufs:
            self.lib.rt_device_free(self.ctx, b)


def test_interleaving(renderer, scene_100):
    """A session at 12x7 with an rt_render_async and an rt_render_split_async of another camera and seed queued
    between its extends on the same context, without a collect in between: they share the counter, scratch and
    camera tables, not the session's records.  Then a session on a second stream after a render on the null
    stream.  Every image equals its own single render."""
    cams = [cam_for(12, 7), cam_for(12, 7, center=(13.0, 3.0, -8.0))]
    npx, lib = 12 * 7, renderer.lib
    renderer.flags = F32
    want = {}
    for n in (128, 384):
        renderer.seed = 11
        want[n] = renderer.render_flat(50, n, scene_100, cams[0], want_linear=True)[1]
    renderer.seed = 22
    other = renderer.render_flat(50, 384, scene_100, cams[1], want_linear=True)[1]
    hip = ctypes.CDLL("libamdhip64.so.7")
    second = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(second)) == 0
    raw = Raw(renderer, scene_100, npx)
    tr = abi.RtTileRange(0, 1, 7, 0, 12)
    try:
        for streams in ((None, None), (None, second)):
            abi.check(lib, lib.rt_progressive_begin(renderer.ctx, ctypes.byref(cams[0]), 50, 384, 11, F32, ctypes.byref(tr), 0))
            try:
                b128 = raw.extend(128, streams[1])
                u = raw.render(cams[1], 50, 384, 22, F32, streams[0], None)
                v = raw.render(cams[1], 50, 384, 22, F32, streams[0], 128)
                b384 = raw.extend(384, streams[1])
                st = raw.collect(streams[1])
                assert st.samples == npx * 384 * 3 and st.pixels == npx * 4
                np.testing.assert_array_equal(raw.read(b128), want[128], err_msg=str(streams))
                np.testing.assert_array_equal(raw.read(b384), want[384], err_msg=str(streams))
                np.testing.assert_array_equal(raw.read(u), other, err_msg=str(streams))
                np.testing.assert_array_equal(raw.read(v), other, err_msg=str(streams))
            finally:
                abi.check(lib, lib.rt_progressive_end(renderer.ctx))
    finally:
        raw.close()
        hip.hipStreamDestroy(second)


# ---- 14. RT_ERR_RANGE ----
def test_range_error(renderer):
    """A white scene: RT_ERR_RANGE is reported at the snapshot's collect and the image is still written (it
    equals the oracle's, which check_snapshot compares)."""
    flat = rt.FlatScene(np.array([[0.0, 0.0, 0.0]]), np.array([5.0]), np.array([0], np.uint32),
                        [rt.Lambertian((9.0, 9.0, 9.0))])
    run_schedule(renderer, ("hot",), flat, cam_for(16, 9), 4, 8, [4, 8], 0, rc_want=abi.RT_ERR_RANGE)


# ---- 15. refusals ----
def test_refusals(renderer, scene_100):
    lib, ctx = renderer.lib, renderer.ctx
    renderer.set_scene(scene_100)
    cam = cam_for(8, 4)
    tr = abi.RtTileRange(0, 1, 4, 0, 8)

    def begin(cap=64, flags=0, depth=8, c=cam, t=tr, max_bytes=0):
        return lib.rt_progressive_begin(ctx, ctypes.byref(c), depth, cap, SEED, flags, ctypes.byref(t), max_bytes)

    def extend(n):
        return lib.rt_progressive_extend_async(ctx, n, None, None, None)

    def refused(rc, code, who):
        assert rc == code, (rc, lib.rt_last_error())
        assert who in lib.rt_last_error(), lib.rt_last_error()

    # no session open
    refused(extend(16), abi.RT_ERR_INVALID, b"rt_progressive_extend_async")
    refused(lib.rt_progressive_end(ctx), abi.RT_ERR_INVALID, b"rt_progressive_end")
    # begin: the live path only, and the limits
    for flags in (abi.RT_FLAG_ROOT2, abi.RT_FLAG_ROOT2 | F32, abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR,
                  abi.RT_FLAG_MODE_VECTORIZED3):
        refused(begin(flags=flags), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_begin")
    refused(begin(cap=(1 << 20) + 1), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_begin")
    refused(begin(flags=F32, depth=abi.RT_MAX_BOUNCES_F32 + 1), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_begin")
    refused(begin(cap=0), abi.RT_ERR_INVALID, b"rt_progressive_begin")
    refused(begin(max_bytes=1024), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_begin")     # 32 regions of 2304 bytes
    big = cam_for(1024, 1024)
    refused(begin(cap=2048, flags=F32, c=big, t=abi.RtTileRange(0, 1, 1024, 0, 1024)), abi.RT_ERR_UNSUPPORTED,
            b"rt_progressive_begin")                                                     # 36.5 GB over the 24 GB budget
    huge = cam_for(65536, 32768)   # 2^31 pixels: an extend has one item per pixel at least, 0x7FFFFFFF at most
    refused(begin(cap=1, c=huge, t=abi.RtTileRange(0, 1, 32768, 0, 65536)), abi.RT_ERR_UNSUPPORTED, b"rt_progressive_begin")
    refused(extend(16), abi.RT_ERR_INVALID, b"rt_progressive_extend_async")              # none of them opened one
    # an open session
    assert begin() == abi.RT_OK
    try:
        refused(begin(), abi.RT_ERR_INVALID, b"rt_progressive_begin")
        refused(lib.rt_context_set_scene(ctx, ctypes.byref(scene_100.abi)), abi.RT_ERR_INVALID, b"rt_context_set_scene")
        refused(extend(0), abi.RT_ERR_INVALID, b"rt_progressive_extend_async")
        refused(extend(65), abi.RT_ERR_INVALID, b"rt_progressive_extend_async")
        assert extend(16) == abi.RT_OK                                                  # trace only
        st = abi.RtStats()
        assert lib.rt_context_collect(ctx, None, ctypes.byref(st)) == abi.RT_OK and st.samples == 32 * 16
        refused(extend(8), abi.RT_ERR_INVALID, b"rt_progressive_extend_async")          # below done
        assert extend(16) == abi.RT_OK                                                  # nothing to do
    finally:
        assert lib.rt_progressive_end(ctx) == abi.RT_OK
    refused(lib.rt_progressive_end(ctx), abi.RT_ERR_INVALID, b"rt_progressive_end")
    st = abi.RtStats()
    assert lib.rt_context_collect(ctx, None, ctypes.byref(st)) == abi.RT_OK
    assert st.samples == 0 and st.kernel_id == 0   # nothing was enqueued
    renderer.set_scene(scene_100)                   # allowed again


def test_destroy_ends_a_session(lib, scene_100):
    """rt_context_destroy with a session open frees it; a closed renderer's session refuses further use."""
    r = rt.GpuRenderer(lib=lib, precision="f32")
    s = r.begin_progressive(8, 64, scene_100, cam_for(8, 4))
    s.extend(16, image=False)
    r.close()
    with pytest.raises(RuntimeError):
        s.extend(32)
    s.close()   # no call into the destroyed context


# ---- 16. Python and CLI ----
def test_renderer_progressive(lib):
    """GpuRenderer.progressive: one image per step, each equal to render() at that spp."""
    scene = rt.scenes.three_spheres()
    cam = rt.Camera(16, 9, **rt.MAIN_CAMERA)
    a = rt.GpuRenderer(lib=lib, precision="f32")
    b = rt.GpuRenderer(lib=lib, precision="f32")
    try:
        steps = list(a.progressive(8, [16, 64, 1024], scene, cam))
        assert [s[0] for s in steps] == [16, 64, 1024]
        total = 0
        for (n, img, stat), prev in zip(steps, (0, 16, 64)):
            want, wstat = b.render(8, n, scene, cam)
            assert img.shape == (9, 16, 3) and img.dtype == np.uint8
            np.testing.assert_array_equal(img, want)
            total += stat.ray_segments
            assert total == wstat.ray_segments and stat.samples == 16 * 9 * (n - prev) and not stat.range_error
        # the generator closed its session: the context takes another
        assert [s[0] for s in a.progressive(8, [4], scene, cam)] == [4]
    finally:
        a.close()
        b.close()


def test_renderer_progressive_reports_range_error(lib):
    """RT_ERR_RANGE at a step is a flag on the yielded stat, not an exception (render() raises)."""
    hot = rt.FlatScene(np.array([[0.0, 0.0, 0.0]]), np.array([5.0]), np.array([0], np.uint32), [rt.Lambertian((9.0, 9.0, 9.0))])
    r = rt.GpuRenderer(lib=lib)
    try:
        steps = list(r.progressive(4, [4, 8], hot, cam_for(16, 9)))
        assert len(steps) == 2 and all(stat.range_error for _, _, stat in steps)
        with pytest.raises(rt.RtError):
            r.render(4, 8, hot, cam_for(16, 9))
    finally:
        r.close()


def test_cli_progressive(tmp_path):
    """rt-render --progressive 16,64 --spp 1024: three files; the final one and the 16 spp one equal the oracle's
    images, and the final one equals the file the same command writes without --progressive."""
    cli = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-ray-tracing_amd", "bin", "rt-render")
    scene = rt.scenes.three_spheres()
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(scene))
    args = [cli, "--width", "16", "--height", "9", "--spp", "1024", "--bounces", "8", "--f32"]
    r = subprocess.run(args + ["--progressive", "16,64", "--out", "o.ppm"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.glob("*.ppm")) == ["o.ppm", "o_spp0000016.ppm", "o_spp0000064.ppm"]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Progressive: ")]
    assert len(lines) == 2 and "16 spp" in lines[0] and "64 spp" in lines[1] and "Msamples/s" in lines[0]
    for name, spp in (("o.ppm", 1024), ("o_spp0000016.ppm", 16)):
        raw = (tmp_path / name).read_bytes()
        assert raw.startswith(b"P6")
        want, _, segs, rc = oracle_render(scene.flatten(), cam_for(16, 9), 8, spp, SEED, precision="f32")
        assert rc == 0
        np.testing.assert_array_equal(np.frombuffer(raw[-16 * 9 * 3:], np.uint8).reshape(-1, 3), want)
    total = oracle_render(scene.flatten(), cam_for(16, 9), 8, 1024, SEED, precision="f32")[2]
    assert f"{total} ray segments" in r.stdout
    r2 = subprocess.run(args + ["--out", "plain.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0, r2.stderr
    assert (tmp_path / "plain.ppm").read_bytes() == (tmp_path / "o.ppm").read_bytes()
