"""The sample-parallel path (rt_render_split_async: trace_paths_split over (pixel, sample sub-range) items,
then finish_records) against the CPU oracle and against the same render through rt_render_async.

Bar: 0 ulp.  Every case compares the linear image, the RGB8 bytes, ray_segments and the return code bit for
bit with oracle_render, and the image, ray_segments and bounce_iters with the unsplit render; where the split
is forced, RT_KERNEL_SPLIT(kernel_id) must be set.  The shapes are the smallest at which each part can go
wrong (ragged last items, items ending inside a camera batch, every record format, both camera paths, the
mega kernels, K > 64); frames the oracle cannot render in test time are checked on a strided pixel subset.
"""
import ctypes

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


@pytest.fixture(scope="module")
def scene_e():
    return rt.scenes.config_scene("E").flatten()


def tile_pixels(cam, tile):
    """Global pixel indices of a tile range, in the output's order."""
    rows = tile.row_begin + np.arange(tile.row_count, dtype=np.int64) * tile.row_step
    cols = tile.col_begin + np.arange(tile.col_count, dtype=np.int64)
    return (rows[:, None] * cam.image_width + cols[None, :]).reshape(-1).astype(np.uint32)


_refs = {}


def reference(key, flat, cam, depth, spp, flags, pixels=None, seed=SEED):
    """oracle_render, computed once per key and shared by the cases that differ only in the split."""
    if key not in _refs:
        r = oracle_render(flat, cam, depth, spp, seed, 0, pixels=pixels, precision="f32" if flags & F32 else "f64")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def run(renderer, flat, cam, depth, spp, flags, S, tile=None, seed=SEED):
    renderer.seed, renderer.flags = seed, flags
    return renderer.render_flat(depth, spp, flat, cam, tile_range=tile, want_linear=True, samples_per_item=S)


def check(renderer, key, flat, cam, depth, spp, flags, S, tile=None, subset=None, rc_want=None):
    """One case: split (S: 0 auto, n forced) against the oracle and against the unsplit render.
    subset: compare with the oracle on these output indices only (frames too large for the oracle).
    The return code is the oracle's (RT_ERR_RANGE is legitimate: at 1 spp the three missing lanes of the
    chunk add sky(0) to the pixel before / spp); rc_want pins it where the case is about it."""
    ukey = ("unsplit",) + key
    if ukey not in _refs:
        _refs[ukey] = run(renderer, flat, cam, depth, spp, flags, None, tile)
    rgb_u, lin_u, st_u, rc_u = _refs[ukey]
    rgb_s, lin_s, st_s, rc_s = run(renderer, flat, cam, depth, spp, flags, S, tile)
    px = tile_pixels(cam, tile) if tile is not None else None
    if subset is not None:
        allpx = px if px is not None else np.arange(cam.image_width * cam.image_height, dtype=np.uint32)
        rgb_o, lin_o, segs_o, rc_o = reference(key, flat, cam, depth, spp, flags, pixels=allpx[subset])
        np.testing.assert_array_equal(lin_s[subset], lin_o)
        np.testing.assert_array_equal(rgb_s[subset], rgb_o)
    else:
        rgb_o, lin_o, segs_o, rc_o = reference(key, flat, cam, depth, spp, flags, pixels=px)
        bad = np.argwhere(lin_s != lin_o)
        assert bad.size == 0, f"{len(bad)} channels differ from the oracle; first pixel {bad[0][0]}: " \
                              f"{lin_s[bad[0][0]]} / {lin_o[bad[0][0]]}"
        np.testing.assert_array_equal(rgb_s, rgb_o)
        assert st_s.ray_segments == segs_o
        assert rc_s == rc_o
    assert rc_s == rc_u and (rc_want is None or rc_s == rc_want)
    np.testing.assert_array_equal(lin_s, lin_u)
    np.testing.assert_array_equal(rgb_s, rgb_u)
    assert (st_s.ray_segments, st_s.bounce_iters, st_s.samples, st_s.pixels) == \
           (st_u.ray_segments, st_u.bounce_iters, st_u.samples, st_u.pixels)
    assert st_s.direct_sky_samples == 0 or not abi.RT_KERNEL_SPLIT(st_s.kernel_id)
    assert not abi.RT_KERNEL_SPLIT(st_u.kernel_id)
    if S:
        assert abi.RT_KERNEL_SPLIT(st_s.kernel_id), hex(st_s.kernel_id)
        k = abi.kernel_info(st_s.kernel_id)
        assert k["T"] == ("float" if flags & F32 else "double") and k["W"] == (5 if flags & F32 else 4)
        assert st_s.kernel_wg_per_cu >= k["W"]
    return st_s, st_u


def auto_plan(lib, n_pixels, spp, flags):
    """The plan rt_render_split_async makes on an MI355X: 256 CUs x 4 SIMDs x the split kernels' waves."""
    s, n = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.rt_split_plan(n_pixels, spp, 256 * 4 * (5 if flags & F32 else 4), ctypes.byref(s), ctypes.byref(n)) == 0
    return s.value, n.value


# ---- sub-range edges ----
@pytest.mark.parametrize("flags", [0, F32])
@pytest.mark.parametrize("spp,S", [(512, 128), (512, 64), (512, 100), (512, 7), (512, 1), (512, 512), (512, 4096),
                                   (6, 4), (6, 1), (100, 64), (1, 1)])
def test_sub_range_edges(renderer, scene_100, spp, S, flags):
    """4x3: a ragged last item (100, 7), items ending inside a 64-sample camera batch (100, 7, 1), S >= spp
    (one item per pixel through the split kernels), a partial chunk (6), (C-1)%2 == 0 (100), one sample."""
    check(renderer, ("edges", spp, flags), scene_100, cam_for(4, 3), 50, spp, flags, S)


# ---- one pixel, the whole chip ----
@pytest.mark.parametrize("flags", [0, F32])
def test_one_pixel_4096(renderer, lib, scene_100, flags):
    S, n_items = auto_plan(lib, 1, 4096, flags)
    assert n_items > 1 and S % 128 == 0
    tile = abi.RtTileRange(20, 1, 1, 30, 1)   # a pixel on the spheres
    st, _ = check(renderer, ("one", 4096, flags), scene_100, cam_for(64, 36), 50, 4096, flags, 0, tile=tile)
    assert abi.RT_KERNEL_SPLIT(st.kernel_id)


def test_one_pixel_at_the_spp_limit(renderer, lib, scene_100):
    """1x1 at the ABI's 2^20 spp, fp32, auto: 8 192 items of 128 samples."""
    assert auto_plan(lib, 1, 1 << 20, F32) == (128, 8192)
    st, _ = check(renderer, ("one", 1 << 20), scene_100, cam_for(1, 1), 50, 1 << 20, F32, 0)
    assert abi.RT_KERNEL_SPLIT(st.kernel_id)


# ---- record formats ----
@pytest.mark.parametrize("spp,flags", [(70001, F32), (32761, F32), (32765, 0)])
def test_wide_position_maps(renderer, scene_100, spp, flags):
    """P = 70004 (u32 map), 32764 (the last u16 map) and 32768 (the first u32 map), as test_wide_records."""
    check(renderer, ("wide", spp, flags), scene_100, cam_for(2, 1), 50, spp, flags, 128 * 37)
    check(renderer, ("wide", spp, flags), scene_100, cam_for(2, 1), 50, spp, flags, 0)


def test_wide_termination_bounces(renderer, scene_100):
    """depth 300 > 254: u32 termination bounces in the record buffer."""
    check(renderer, ("e32",), scene_100, cam_for(16, 9), 300, 256, 0, 128)


# ---- paths ----
@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("flags", [0, F32])
def test_depth_edges(renderer, scene_100, depth, flags):
    check(renderer, ("depth", depth, flags), scene_100, cam_for(8, 5), depth, 256, flags, 128)


@pytest.mark.parametrize("flags", [0, F32])
def test_defocus_camera(renderer, scene_100, flags):
    """The kernels without camera batches (every primary ray has its own origin)."""
    st, _ = check(renderer, ("defocus", flags), scene_100, cam_for(8, 5, defocus_angle=2.0), 50, 256, flags, 128)
    assert not abi.kernel_info(st.kernel_id)["camq"]


@pytest.mark.parametrize("flags", [0, F32])
def test_sky_only(renderer, scene_100, flags):
    """The empty scene, and a camera that sees no sphere.  rt_render_async finishes the empty scene's pixels
    when it claims them (direct sky); the split kernels trace them and every sample writes e = 0."""
    _, st_u = check(renderer, ("empty", flags), EMPTY(), cam_for(8, 5), 50, 512, flags, 128)
    assert st_u.direct_sky_samples == 8 * 5 * 512
    up = cam_for(8, 5, center=(0.0, 30.0, 0.0), look_at=(3.0, 60.0, 1.0))
    st_s, st_u = check(renderer, ("sky", flags), scene_100, up, 50, 512, flags, 128)
    assert st_s.ray_segments == 8 * 5 * 512   # one segment per sample: every primary ray escapes


@pytest.mark.parametrize("flags,spp", [(F32, 2048), (0, 256)])
def test_config_e_scene(renderer, scene_e, flags, spp):
    """Config E's 10 000 spheres: the mega kernels."""
    st, _ = check(renderer, ("E", flags), scene_e, cam_for(4, 3), 50, spp, flags, 128)
    assert abi.kernel_info(st.kernel_id)["mega"]


def cage():
    """Six large fuzzy-mirror spheres that overlap around the camera (their surfaces 3 units away on every
    side).  A ray bounces between them until a fuzzed reflection leaves through a seam: on the oracle the
    mean path is ~132 bounces of 200 in both precisions and no pixel's mean is under 96, so short paths and
    paths that last all 200 bounces mix in every pixel and every pixel has K > 64."""
    c = np.array(rt.MAIN_CAMERA["center"])
    off = [(103.0, 0, 0), (-103.0, 0, 0), (0, 0, 103.0), (0, 0, -103.0), (0, -103.0, 0), (0, 103.0, 0)]
    return rt.FlatScene(np.array([c + np.array(o) for o in off]), np.full(6, 100.0), np.zeros(6, np.uint32),
                        [rt.Metal((0.97, 0.95, 0.9), 0.3)])


@pytest.mark.parametrize("flags", [0, F32])
def test_long_paths(renderer, flags):
    """K > 64: finish_pixel's per-bounce replay (the bit-plane replay covers K <= 64) on split records.
    test_long_paths_replay's glass sphere traps rays only with RT_FLAG_ROOT2, which this path refuses, so the
    long paths here come from a cage of mirrors on the live path; that scene is rendered too (every primary
    ray starts inside the sphere and misses it: quirk Q1)."""
    flat = cage()
    st_s, st_u = check(renderer, ("cage", flags), flat, cam_for(16, 9), 200, 24, flags, 8)
    # each pixel's K = min(depth, longest path + 1) is at least its mean path: the K > 64 replay ran, on
    # records that mix early and late terminations (fewer segments than 200 per sample)
    assert st_u.bounce_iters > 64 * 16 * 9 and st_u.ray_segments < 160 * 16 * 9 * 24
    tir = rt.FlatScene(np.array([[16.0, 2.0, 56.5]]), np.array([40.0]), np.array([0], np.uint32), [rt.Dielectric(1.5, False)])
    check(renderer, ("tir", flags), tir, cam_for(16, 9), 200, 24, flags, 8)


def test_range_error(renderer):
    """A white scene: RT_ERR_RANGE from rt_context_collect, the image still written."""
    flat = rt.FlatScene(np.array([[0.0, 0.0, 0.0]]), np.array([5.0]), np.array([0], np.uint32),
                        [rt.Lambertian((9.0, 9.0, 9.0))])
    check(renderer, ("hot",), flat, cam_for(16, 9), 4, 8, 0, 4, rc_want=abi.RT_ERR_RANGE)


# ---- scheduling ----
def test_thumbnail_auto(renderer, lib, scene_100):
    S, n_items = auto_plan(lib, 64 * 36, 512, F32)
    assert n_items > 64 * 36
    st, _ = check(renderer, ("thumb",), scene_100, cam_for(64, 36), 50, 512, F32, 0)
    assert abi.RT_KERNEL_SPLIT(st.kernel_id)


def test_one_item_per_pixel_large_frame(renderer, scene_100):
    """1280x720 at 16 spp with S = 128: 921 600 single-item pixels through the split kernels (guided blocks
    of 16, every claim stream).  Oracle on 2 048 strided pixels, the whole frame against rt_render_async."""
    subset = (np.arange(2048, dtype=np.int64) * 449) % (1280 * 720)
    check(renderer, ("720p",), scene_100, cam_for(1280, 720), 50, 16, F32, 128, subset=subset)


@pytest.mark.parametrize("flags", [0, F32])
def test_row_strided_tile(renderer, scene_100, flags):
    tile = abi.RtTileRange(1, 3, 18, 5, 80)   # rows 1, 4, ..., 52 of 54; columns 5..84 of 96
    check(renderer, ("strided", flags), scene_100, cam_for(96, 54), 50, 256, flags, 128, tile=tile)


# ---- context ordering ----
class Raw:
    """The async API without a collect in between."""

    def __init__(self, renderer, flat, npx):
        self.lib, self.ctx, self.npx = renderer.lib, renderer.ctx, npx
        renderer.set_scene(flat)
        self.bufs = []

    def render(self, cam, depth, spp, seed, flags, stream, S):
        b = ctypes.c_void_p()
        abi.check(self.lib, self.lib.rt_device_alloc(self.ctx, self.npx * 24, ctypes.byref(b)))
        self.bufs.append(b)
        tr = abi.RtTileRange(0, 1, cam.image_height, 0, cam.image_width)
        if S is None:
            rc = self.lib.rt_render_async(self.ctx, ctypes.byref(cam), depth, spp, seed, flags, ctypes.byref(tr), None, b, stream)
        else:
            rc = self.lib.rt_render_split_async(self.ctx, ctypes.byref(cam), depth, spp, seed, flags, ctypes.byref(tr),
                                                None, b, stream, S)
        abi.check(self.lib, rc)
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


def test_context_ordering(renderer, scene_100):
    """Renders that share the context's record buffer, scratch, counters and camera tables, queued without a
    collect in between: two split renders with different cameras; split after unsplit and the reverse; a
    split render on a second stream.  Every image equals its own single render."""
    cams = [cam_for(12, 7), cam_for(12, 7, center=(13.0, 3.0, -8.0))]
    spp, npx = 384, 12 * 7
    want = [run(renderer, scene_100, c, 50, spp, F32, None, seed=s)[1] for c, s in zip(cams, (11, 22))]
    hip = ctypes.CDLL("libamdhip64.so.7")
    second = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(second)) == 0
    raw = Raw(renderer, scene_100, npx)
    try:
        for S0, S1, streams in ((128, 128, (None, None)), (None, 128, (None, None)), (128, None, (None, None)),
                                (128, 64, (None, second))):
            b0 = raw.render(cams[0], 50, spp, 11, F32, streams[0], S0)
            b1 = raw.render(cams[1], 50, spp, 22, F32, streams[1], S1)
            st = raw.collect(streams[1])
            assert st.samples == 2 * npx * spp
            np.testing.assert_array_equal(raw.read(b0), want[0], err_msg=str((S0, S1)))
            np.testing.assert_array_equal(raw.read(b1), want[1], err_msg=str((S0, S1)))
    finally:
        raw.close()
        hip.hipStreamDestroy(second)


# ---- refusals ----
def test_refusals(renderer, scene_100):
    lib = renderer.lib
    renderer.set_scene(scene_100)
    cam = cam_for(8, 4)
    tr = abi.RtTileRange(0, 1, 4, 0, 8)

    def call(spp, flags, S, c=cam, t=tr):
        return lib.rt_render_split_async(renderer.ctx, ctypes.byref(c), 8, spp, SEED, flags, ctypes.byref(t), None, None, None, S)

    for S in (0, 128):
        for flags in (abi.RT_FLAG_ROOT2, abi.RT_FLAG_ROOT2 | F32, abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR,
                      abi.RT_FLAG_MODE_VECTORIZED3):
            assert call(256, flags, S) == abi.RT_ERR_UNSUPPORTED, (flags, S)
            assert b"rt_render_split_async" in lib.rt_last_error()
        assert call(256, 0x20, S) == abi.RT_ERR_INVALID
        assert call(256, abi.RT_FLAG_MODE_VECTORIZED | abi.RT_FLAG_MODE_SCALAR, S) == abi.RT_ERR_INVALID
        assert call(0, 0, S) == abi.RT_ERR_INVALID
        assert call((1 << 20) + 1, F32, S) == abi.RT_ERR_UNSUPPORTED
        assert call(256, F32, S, t=abi.RtTileRange(0, 1, 5, 0, 8)) == abi.RT_ERR_INVALID     # 5 rows of 4
    assert call(256, F32, (1 << 20) + 1) == abi.RT_ERR_INVALID
    # forced: more work items than one launch counts (2^20 pixels x 2^11 items)
    big = cam_for(1024, 1024)
    assert call(1 << 11, F32, 1, c=big, t=abi.RtTileRange(0, 1, 1024, 0, 1024)) == abi.RT_ERR_UNSUPPORTED
    # forced: a record buffer over the 24 GB scratch budget (2^20 pixels x 34 KB)
    assert call(1 << 11, F32, 1 << 10, c=big, t=abi.RtTileRange(0, 1, 1024, 0, 1024)) == abi.RT_ERR_UNSUPPORTED
    st = abi.RtStats()
    assert lib.rt_context_collect(renderer.ctx, None, ctypes.byref(st)) == abi.RT_OK
    assert st.samples == 0 and st.kernel_id == 0   # nothing was enqueued


# ---- auto equals unsplit ----
def test_auto_is_unsplit_on_a_full_frame(renderer, scene_100):
    """1920x1080 at 16 spp: the plan is one item per pixel, so the call is rt_render_async (same kernel)."""
    subset = (np.arange(1024, dtype=np.int64) * 2027) % (1920 * 1080)
    st_s, st_u = check(renderer, ("1080p",), scene_100, cam_for(1920, 1080), 50, 16, F32, 0, subset=subset)
    assert st_s.kernel_id == st_u.kernel_id and not abi.RT_KERNEL_SPLIT(st_s.kernel_id)
    assert st_s.direct_sky_samples == st_u.direct_sky_samples > 0


def test_renderer_sample_parallel(lib):
    """GpuRenderer(sample_parallel=True).render: the Renderer trait's call on the auto plan."""
    scene = rt.scenes.three_spheres()
    cam = rt.Camera(16, 9, **rt.MAIN_CAMERA)
    a = rt.GpuRenderer(lib=lib, precision="f32", sample_parallel=True)
    b = rt.GpuRenderer(lib=lib, precision="f32")
    try:
        img_a, stat_a = a.render(8, 1024, scene, cam)
        img_b, stat_b = b.render(8, 1024, scene, cam)
    finally:
        a.close()
        b.close()
    np.testing.assert_array_equal(img_a, img_b)
    assert stat_a.ray_segments == stat_b.ray_segments and stat_a.samples == 16 * 9 * 1024


def test_cli_sample_parallel(tmp_path):
    """rt-render --sample-parallel: the PPM bytes equal the oracle's image (a 16x9 frame at 1024 spp is split)."""
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-ray-tracing_amd", "bin", "rt-render")
    scene = rt.scenes.three_spheres()
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(scene))
    r = subprocess.run([cli, "--width", "16", "--height", "9", "--spp", "1024", "--bounces", "8", "--f32",
                        "--sample-parallel", "--out", "o.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = (tmp_path / "o.ppm").read_bytes()
    assert raw.startswith(b"P6")
    want, _, segs, rc = oracle_render(scene.flatten(), cam_for(16, 9), 8, 1024, SEED, precision="f32")
    assert rc == 0
    np.testing.assert_array_equal(np.frombuffer(raw[-16 * 9 * 3:], np.uint8).reshape(-1, 3), want)
    assert f"{segs} ray segments" in r.stdout
