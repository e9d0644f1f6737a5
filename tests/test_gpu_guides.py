"""Guide buffers (rt_render_guides_async: guide_pixels<T, CAMQ, MEGA>) against a restatement of their definition.

The reference is the restatement of tests/guide_restatement.py, built on tests/independent_v2.py (imported, not
modified): get_ray gives the primary ray of (pixel, sample, seed), hit_scene the live path's closest hit at
bounce 0 with the finalized normal, scene_from_flat the materials in the render's precision, and fold() is the
definition's reduction in numpy.  Per-sample values do not depend on the sample count, so each frame's samples
are restated once, at the largest count a test needs, and every smaller count folds a prefix of them.

Bar: 0 ulp.  Every comparison is np.testing.assert_array_equal on the float32 arrays.

Shapes are the smallest at which each part can go wrong: one live lane, a partial batch, a full batch, a second
batch with one live lane, three batches with a ragged end; both camera paths; an empty candidate list; the three
material kinds and quirk Q1; the mega kernels; a strided range; more pixels than a launch has waves.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt_mi355x as rt
from rt_mi355x import abi
from guide_restatement import SEED, _refs, restate_guides, restate_samples, samples_once

pytestmark = pytest.mark.gpu

F32 = abi.RT_FLAG_F32
NAMES = ("albedo", "normal", "depth", "coverage")
PRECS = ("f64", "f32")
CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-ray-tracing_amd", "bin", "rt-render")


def guides(renderer, prec, spp, flat, cam, tile=None, want=NAMES, seed=SEED):
    renderer.seed, renderer.flags = seed, F32 if prec == "f32" else 0
    out, st, rc = renderer.guides_flat(spp, flat, cam, tile_range=tile, want=want)
    assert rc == abi.RT_OK
    for name in want:
        assert out[name].dtype == np.float32
    return out, st


def assert_guides_equal(got, want, names=NAMES):
    for name in names:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def check_stats(st, npx, spp, prec, camq, mega):
    k = abi.kernel_info(st.kernel_id)
    assert abi.RT_KERNEL_GUIDES(st.kernel_id) == 1 and k["guides"]
    assert k["camq"] is camq and k["mega"] is mega and k["T"] == ("float" if prec == "f32" else "double")
    assert not k["split"] and not k["items"] and not k["root2"] and k["mode"] == 0
    assert abi.kernel_name(st.kernel_id).startswith("guide_pixels<")
    assert st.pixels == npx and st.samples == npx * spp and st.ray_segments == npx * spp
    assert st.bounce_iters == 0
    assert st.kernel_wg_per_cu >= 1 and st.kernel_ms > 0


def cam_for(w, h, **kw):
    return rt.camera_new_py(w, h, **dict(rt.MAIN_CAMERA, **kw))


@pytest.fixture(scope="module")
def scene_100():
    return rt.scenes.random_spheres(100).flatten()


def material_scene():
    """One Lambertian, one Metal (fuzz 0.3) and one hollow Dielectric sphere side by side over a Lambertian ground."""
    return rt.Scene.from_list([
        rt.Sphere((0.0, -1000.0, 0.0), 1000.0, rt.Lambertian((0.5, 0.5, 0.5))),
        rt.Sphere((-4.0, 1.0, 0.0), 1.0, rt.Lambertian((0.4, 0.2, 0.1))),
        rt.Sphere((0.0, 1.0, 0.0), 1.0, rt.Metal((0.7, 0.6, 0.5), 0.3)),
        rt.Sphere((4.0, 1.0, 0.0), 1.0, rt.Dielectric(1.5, True)),
    ])


EMPTY = lambda: rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32),   # noqa: E731
                             [rt.Lambertian((0.5, 0.5, 0.5))])


# ---------------------------------------------------------------- 1. batches
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("spp", [1, 6, 64, 65, 130])
def test_batches(renderer, scene_100, prec, spp):
    """16x9, 100 spheres, pinhole: one live lane, a partial batch, a full batch, a second batch with one live lane,
    three batches with a ragged end."""
    cam = cam_for(16, 9)
    vals, _ = samples_once(("batches", prec), scene_100, cam, 130, prec)
    got, st = guides(renderer, prec, spp, scene_100, cam)
    assert got["albedo"].shape == (144, 3) and got["normal"].shape == (144, 3)
    assert got["depth"].shape == (144,) and got["coverage"].shape == (144,)
    assert_guides_equal(got, restate_guides(vals, spp))
    check_stats(st, 144, spp, prec, camq=True, mega=False)


# ---------------------------------------------------------------- 2. defocus
@pytest.mark.parametrize("prec", PRECS)
def test_defocus(renderer, scene_100, prec):
    """The same frame through a lens: every ray has an origin of its own, so no camera batches (camq false)."""
    cam = cam_for(16, 9, defocus_angle=0.6)
    vals, idx = samples_once(("defocus", prec), scene_100, cam, 65, prec)
    assert (idx >= 0).any() and (idx < 0).any()
    got, st = guides(renderer, prec, 65, scene_100, cam)
    assert_guides_equal(got, restate_guides(vals, 65))
    check_stats(st, 144, 65, prec, camq=False, mega=False)


# ---------------------------------------------------------------- 3. sky
@pytest.mark.parametrize("prec", PRECS)
def test_sky(renderer, scene_100, prec):
    """No hit: albedo exactly 1, normal, depth and coverage exactly 0 (an empty scene; the sky pixels of case 1)."""
    got, st = guides(renderer, prec, 5, EMPTY(), cam_for(8, 8))
    np.testing.assert_array_equal(got["albedo"], np.ones((64, 3), np.float32))
    np.testing.assert_array_equal(got["normal"], np.zeros((64, 3), np.float32))
    np.testing.assert_array_equal(got["depth"], np.zeros(64, np.float32))
    np.testing.assert_array_equal(got["coverage"], np.zeros(64, np.float32))
    assert not np.signbit(got["normal"]).any() and not np.signbit(got["depth"]).any()
    check_stats(st, 64, 5, prec, camq=True, mega=False)
    cam = cam_for(16, 9)
    vals, _ = samples_once(("batches", prec), scene_100, cam, 130, prec)
    want = restate_guides(vals, 65)
    sky = want["coverage"] == 0
    assert sky.any()
    got, _ = guides(renderer, prec, 65, scene_100, cam)
    np.testing.assert_array_equal(got["albedo"][sky], np.ones((sky.sum(), 3), np.float32))
    for name in ("normal", "depth", "coverage"):
        assert not got[name][sky].any(), name


# ---------------------------------------------------------------- 4. materials and Q1
@pytest.mark.parametrize("prec", PRECS)
def test_materials(renderer, prec):
    """Lambertian and Metal give their albedo, a Dielectric 1; 24x8 x 6 spp over all three."""
    flat = material_scene().flatten()
    cam = cam_for(24, 8)
    vals, idx = samples_once(("materials", prec), flat, cam, 6, prec)
    assert {1, 2, 3} <= set(np.unique(idx).tolist())
    got, st = guides(renderer, prec, 6, flat, cam)
    assert_guides_equal(got, restate_guides(vals, 6))
    check_stats(st, 192, 6, prec, camq=True, mega=False)


def test_camera_inside_a_sphere(renderer):
    """Quirk Q1: from inside a sphere the near root is invalid and the far one is never taken, so the enclosing
    sphere is not hit; a small sphere in front still is.  The guides follow the render's behaviour."""
    flat = rt.Scene.from_list([
        rt.Sphere((0.0, 0.0, 0.0), 50.0, rt.Lambertian((0.2, 0.3, 0.4))),
        rt.Sphere((0.0, 0.0, -5.0), 1.0, rt.Metal((0.9, 0.8, 0.7), 0.0)),
    ]).flatten()
    cam = rt.camera_new_py(8, 8, focal_length=1.0, view_angle=40.0, center=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0),
                           up=(0.0, 1.0, 0.0), defocus_angle=0.0)
    vals, idx = restate_samples(flat, cam, 4, "f64")
    assert (idx == 1).any() and (idx == -1).any() and not (idx == 0).any()
    got, _ = guides(renderer, "f64", 4, flat, cam)
    assert_guides_equal(got, restate_guides(vals, 4))


# ---------------------------------------------------------------- 5. mega
@pytest.mark.parametrize("prec", PRECS)
def test_mega(renderer, prec):
    """10 000 spheres: the MEGA instantiations (the super level of the cone walk)."""
    if "E" not in _refs:
        _refs["E"] = rt.scenes.config_scene("E").flatten()
    flat = _refs["E"]
    cam = cam_for(16, 9)
    vals, idx = samples_once(("mega", prec), flat, cam, 6, prec)
    assert len(np.unique(idx)) > 8
    got, st = guides(renderer, prec, 6, flat, cam)
    assert_guides_equal(got, restate_guides(vals, 6))
    check_stats(st, 144, 6, prec, camq=True, mega=True)


# ---------------------------------------------------------------- 6. range
@pytest.mark.parametrize("prec", PRECS)
def test_range(renderer, scene_100, prec):
    """A strided tile gives the same pixels of the full-frame call, bit for bit, compact over the range."""
    cam = cam_for(16, 9)
    tile = abi.RtTileRange(row_begin=1, row_step=2, row_count=4, col_begin=3, col_count=7)
    full, _ = guides(renderer, prec, 6, scene_100, cam)
    part, st = guides(renderer, prec, 6, scene_100, cam, tile=tile)
    rows = 1 + 2 * np.arange(4)
    px = (rows[:, None] * 16 + (3 + np.arange(7))[None, :]).reshape(-1)
    for name in NAMES:
        assert part[name].shape[0] == 28
        np.testing.assert_array_equal(part[name], full[name][px], err_msg=name)
    check_stats(st, 28, 6, prec, camq=True, mega=False)


# ---------------------------------------------------------------- 7. pixel loop
def test_pixel_loop(renderer, scene_100):
    """640x360 x 2 spp: more pixels than a launch has waves resident, so every wave walks several."""
    cam = cam_for(640, 360)
    got, st = guides(renderer, "f32", 2, scene_100, cam)
    check_stats(st, 640 * 360, 2, "f32", camq=True, mega=False)
    px = np.arange(0, 640 * 360, 900)
    assert len(px) == 256
    vals, idx = restate_samples(scene_100, cam, 2, "f32", pixels=px)
    assert (idx >= 0).any() and (idx < 0).any()
    want = restate_guides(vals, 2)
    for name in NAMES:
        np.testing.assert_array_equal(got[name][px], want[name], err_msg=name)
    assert (got["coverage"] >= 0).all() and (got["coverage"] <= 1).all()
    for name in NAMES:
        assert np.isfinite(got[name]).all(), name


# ---------------------------------------------------------------- 8. output subsets
@pytest.mark.parametrize("prec", PRECS)
def test_output_subsets(renderer, scene_100, prec):
    """A value does not depend on which other outputs were asked for."""
    cam = cam_for(16, 9)
    full, _ = guides(renderer, prec, 6, scene_100, cam)
    for name in NAMES:
        one, st = guides(renderer, prec, 6, scene_100, cam, want=(name,))
        assert list(one) == [name]
        np.testing.assert_array_equal(one[name], full[name], err_msg=name)
        check_stats(st, 144, 6, prec, camq=True, mega=False)
    two, _ = guides(renderer, prec, 6, scene_100, cam, want=("depth", "albedo"))
    assert_guides_equal(two, full, names=("depth", "albedo"))


# ---------------------------------------------------------------- 9. no interference
def test_cameras_do_not_mix(renderer, scene_100):
    """Render with camera A, guides with camera B, render with A: the images are identical (no stale camera table
    either way) and the guides are B's."""
    cam_a = cam_for(16, 9)
    cam_b = cam_for(16, 9, center=(-10.0, 3.0, 14.0))
    renderer.seed, renderer.flags = SEED, 0
    first = renderer.render_flat(8, 4, scene_100, cam_a, want_linear=True)
    got, _ = guides(renderer, "f64", 6, scene_100, cam_b)
    renderer.seed, renderer.flags = SEED, 0
    again = renderer.render_flat(8, 4, scene_100, cam_a, want_linear=True)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    vals, idx = restate_samples(scene_100, cam_b, 6, "f64")
    assert (idx >= 0).any()
    assert_guides_equal(got, restate_guides(vals, 6))


@pytest.mark.parametrize("prec", PRECS)
def test_inside_a_progressive_session(renderer, scene_100, prec):
    """A guide call between two extends touches neither the session's records nor its counts."""
    cam = cam_for(16, 9)
    renderer.seed, renderer.flags = SEED, F32 if prec == "f32" else 0
    want = renderer.render_flat(8, 16, scene_100, cam, want_linear=True)
    alone, _ = guides(renderer, prec, 6, scene_100, cam)
    with renderer.begin_progressive(8, 16, scene_100, cam) as s:
        s.extend(8, image=False)
        before = s.counts
        inside, st = guides(renderer, prec, 6, scene_100, cam)
        check_stats(st, 144, 6, prec, camq=True, mega=False)
        np.testing.assert_array_equal(s.counts, before)
        assert (before == 8).all()
        rgb, lin, _, rc = s.extend(16, want_linear=True)
    assert rc == want[3]
    np.testing.assert_array_equal(rgb, want[0])
    np.testing.assert_array_equal(lin, want[1])
    assert_guides_equal(inside, alone)


# ---------------------------------------------------------------- 10. refusals on a live context
def test_refusals_on_a_live_context(renderer, scene_100):
    lib, ctx = renderer.lib, renderer.ctx
    cam = cam_for(4, 3)
    good, _ = guides(renderer, "f32", 3, scene_100, cam)
    buf = ctypes.c_void_p()
    abi.check(lib, lib.rt_device_alloc(ctx, 12 * 3 * 4, ctypes.byref(buf)))

    def call(spp, flags):
        return lib.rt_render_guides_async(ctx, ctypes.byref(cam), spp, SEED, flags, None, buf, None, None, None, None)

    try:
        cases = [(3, abi.RT_FLAG_ROOT2, abi.RT_ERR_UNSUPPORTED), (3, F32 | abi.RT_FLAG_ROOT2, abi.RT_ERR_UNSUPPORTED),
                 (3, abi.RT_FLAG_MODE_VECTORIZED, abi.RT_ERR_UNSUPPORTED), (3, abi.RT_FLAG_MODE_SCALAR, abi.RT_ERR_UNSUPPORTED),
                 (3, abi.RT_FLAG_MODE_VECTORIZED3, abi.RT_ERR_UNSUPPORTED), (3, 0x20, abi.RT_ERR_INVALID),
                 (3, F32 | 0x20, abi.RT_ERR_INVALID), (0, F32, abi.RT_ERR_INVALID),
                 ((1 << 20) + 1, F32, abi.RT_ERR_UNSUPPORTED)]
        for spp, flags, want in cases:
            assert call(spp, flags) == want, (spp, flags)
            assert b"rt_render_guides_async" in lib.rt_last_error()
            st = abi.RtStats()
            abi.check(lib, lib.rt_context_collect(ctx, None, ctypes.byref(st)))
            assert st.kernel_id == 0 and st.samples == 0 and st.pixels == 0, (spp, flags)
            again, _ = guides(renderer, "f32", 3, scene_100, cam)
            assert_guides_equal(again, good)
        bad_range = abi.RtTileRange(0, 1, 4, 0, 4)   # 4 rows of a 3-row image
        assert lib.rt_render_guides_async(ctx, ctypes.byref(cam), 3, SEED, F32, ctypes.byref(bad_range), buf, None, None,
                                          None, None) == abi.RT_ERR_INVALID
    finally:
        lib.rt_device_free(ctx, buf)
    with pytest.raises(ValueError):
        renderer.guides_flat(3, scene_100, cam, want=("albedo", "normals"))


# ---------------------------------------------------------------- 11. CLI
def read_pfm(path):
    raw = open(path, "rb").read()
    magic, dims, scale, data = raw.split(b"\n", 3)
    assert magic in (b"PF", b"Pf") and scale == b"-1.0"
    w, h = (int(x) for x in dims.split())
    ch = 3 if magic == b"PF" else 1
    a = np.frombuffer(data, dtype="<f4")
    assert a.size == w * h * ch
    a = a.reshape((h, w, ch) if ch == 3 else (h, w))
    return a[::-1]   # rows bottom to top


def test_cli_guides(tmp_path, lib):
    """rt-render --guides writes the four PFM files with GpuRenderer.guides' exact values and leaves --out as it is."""
    scene = material_scene()
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(scene))
    args = [CLI, "--scene", "scene.toml", "--width", "24", "--height", "8", "--spp", "6", "--f32"]
    r = subprocess.run(args + ["--guides", "--out", "o.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run(args + ["--out", "plain.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    assert (tmp_path / "o.ppm").read_bytes() == (tmp_path / "plain.ppm").read_bytes()
    g = rt.GpuRenderer(lib=lib, precision="f32")
    try:
        want, stat = g.guides(6, scene, rt.Camera(24, 8, **rt.MAIN_CAMERA))
    finally:
        g.close()
    assert want.albedo.shape == (8, 24, 3) and want.normal.shape == (8, 24, 3)
    assert want.depth.shape == (8, 24) and want.coverage.shape == (8, 24)
    assert stat.samples == 24 * 8 * 6 and 0 < want.coverage.mean() < 1
    for name in NAMES:
        np.testing.assert_array_equal(read_pfm(tmp_path / f"o_{name}.pfm"), getattr(want, name), err_msg=name)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Guides: ")]
    assert len(lines) == 1 and "kernel" in lines[0] and "Msamples/s" in lines[0]
    assert not any(ln.startswith("Guides: ") for ln in plain.stdout.splitlines())
    # with the other live-path modes of the CLI the guides are still the uniform ones at --spp
    for k, mode in enumerate((["--sample-parallel"], ["--progressive", "2"], ["--adaptive", "0.05", "--spp-min", "2"])):
        m = subprocess.run(args + ["--guides", "--out", f"m{k}.ppm"] + mode, cwd=tmp_path, capture_output=True, text=True,
                           timeout=120)
        assert m.returncode == 0, (mode, m.stderr)
        for name in NAMES:
            assert (tmp_path / f"m{k}_{name}.pfm").read_bytes() == (tmp_path / f"o_{name}.pfm").read_bytes(), (mode, name)
    for flag in (["--root2"], ["--mode", "scalar"], ["--block-size", "64"]):
        bad = subprocess.run(args + ["--guides", "--out", "bad.ppm"] + flag, cwd=tmp_path, capture_output=True, text=True,
                             timeout=120)
        assert bad.returncode != 0 and "--guides" in bad.stderr, (flag, bad.stderr)
