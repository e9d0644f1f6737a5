"""rt_render_rays_async on the GPU: full paths for caller-supplied primary rays, at 0 ulp against two references
(tests/ray_render_cases.py; tests/test_ray_render_cases.py checks them against each other without a GPU).

 1. one ray per pixel against reference A (the C oracle under a degenerate camera): 130 pixels (two full batches and a
    partial one), spp 1, 6 and 70, depth 1 and 8, RT_FLAG_ROOT2 off and on, rays that start inside a sphere and rays
    that miss everything, a nonzero pixel_base; the scene with a mega level too;
 2. R = spp with a camera's own rays (independent_v2.get_ray, a pinhole and a defocus camera): rt_render_async's bytes;
 3. arbitrary per-sample rays, directions of every admitted length, against reference B (the Python restatement);
 4. invalid rays: their pixels NaN / black, every other pixel untouched, samples = valid pixels x spp;
 5. a shared origin against per-ray copies of it;  6. a pixel does not depend on the launch's shape;
 7. RT_ERR_RANGE comes back and the image is still written;  8. the kernel id;
 9. torch tensors in place on a torch stream (a child process);  10, 11. rt-render --projection against
    GpuRenderer.render_rays over rt.projections' rays.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import independent_v2 as iv
import ray_render_cases as rc
import rt_mi355x as rt
from query_cases import assert_same
from rt_mi355x import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(HERE, "..", "rust-ray-tracing_amd", "bin", "rt-render")
BASE = rc.PIXEL_BASE


@pytest.fixture(scope="module")
def renderers(lib):
    rs = {prec: rt.GpuRenderer(precision=prec, seed=rc.SEED, lib=lib) for prec in rc.PRECS}
    yield rs
    for r in rs.values():
        r.close()


def check_kernel(st, prec, root2, mega):
    k = abi.kernel_info(st.kernel_id)
    assert abi.RT_KERNEL_RAYS(st.kernel_id) == 1 and k["rays"]
    assert not k["query"] and not k["guides"] and not k["split"] and not k["items"] and not k["camq"] and k["mode"] == 0
    assert k["T"] == ("float" if prec == "f32" else "double") and k["W"] == (6 if prec == "f32" else 4)
    assert k["root2"] is root2 and k["mega"] is mega
    assert st.kernel_wg_per_cu >= k["W"]
    b = lambda v: "true" if v else "false"   # noqa: E731
    assert abi.kernel_name(st.kernel_id) == f"trace_paths_rays<{k['T']},{k['W']},{b(root2)},{b(mega)}>"


# ---------------------------------------------------------------- 1. one ray per pixel, reference A
@pytest.mark.parametrize("root2", (False, True))
@pytest.mark.parametrize("depth", (1, 8))
@pytest.mark.parametrize("spp", (1, 6, 70))
@pytest.mark.parametrize("prec", rc.PRECS)
def test_single_rays_against_the_oracle(renderers, prec, spp, depth, root2):
    flat = rc.scene("s100")
    o, tgt, d = rc.ray_set(prec)
    rgb_a, lin_a, segs_a, rc_a = rc.reference_a(flat, o, tgt, spp, depth, prec, root2)
    rgb, lin, st, code = renderers[prec].render_rays(depth, spp, o, d, flat, pixel_base=BASE, root2=root2, want_linear=True)
    print(prec, spp, depth, root2, "pixels differing:", int((lin != lin_a).any(1).sum()), "segments", st.ray_segments, segs_a)
    assert code == rc_a
    assert_same(lin, lin_a, "linear")
    assert np.array_equal(rgb, rgb_a)
    assert st.ray_segments == segs_a and st.pixels == rc.N_PIX and st.samples == rc.N_PIX * spp
    check_kernel(st, prec, root2, mega=False)


@pytest.mark.parametrize("root2", (False, True))
@pytest.mark.parametrize("prec", rc.PRECS)
def test_single_rays_mega_scene(renderers, prec, root2):
    flat = rc.scene("mega")
    o, tgt, d = rc.ray_set(prec)
    rgb_a, lin_a, segs_a, rc_a = rc.reference_a(flat, o, tgt, 6, 8, prec, root2)
    rgb, lin, st, code = renderers[prec].render_rays(8, 6, o, d, flat, pixel_base=BASE, root2=root2, want_linear=True)
    print(prec, root2, "pixels differing:", int((lin != lin_a).any(1).sum()), "segments", st.ray_segments, segs_a)
    assert code == rc_a
    assert_same(lin, lin_a, "linear")
    assert np.array_equal(rgb, rgb_a) and st.ray_segments == segs_a
    check_kernel(st, prec, root2, mega=True)


# ---------------------------------------------------------------- 2. a camera's own rays: rt_render_async's image
@pytest.mark.parametrize("defocus", (0.0, 0.6))
@pytest.mark.parametrize("prec", rc.PRECS)
def test_camera_rays_give_the_renders_image(renderers, prec, defocus):
    W, H, spp, depth, row, col0, ncol = 96, 54, 6, 8, 30, 10, 76
    flat = rc.scene("s100")
    cam = rt.camera_new_py(W, H, **dict(rt.MAIN_CAMERA, defocus_angle=defocus))
    civ = {"W": W, "H": H, **{k: tuple(getattr(cam, k)) for k in ("center", "ulc", "vu", "vv", "du", "dv")}}
    camp = iv.camera_in(civ, prec)
    T = rc.DTYPES[prec]
    o, d = np.zeros((ncol, spp, 3), T), np.zeros((ncol, spp, 3), T)
    for c in range(ncol):
        for s in range(spp):
            o[c, s], d[c, s] = iv.get_ray(camp, col0 + c, row, s, row * W + col0 + c, rc.SEED, prec)
    assert (defocus == 0.0) == bool((o == o[0, 0]).all())
    r = renderers[prec]
    rgb_w, lin_w, st_w, rc_w = r.render_flat(depth, spp, flat, cam, tile_range=abi.RtTileRange(row, 1, 1, col0, ncol),
                                             want_linear=True)
    rgb, lin, st, code = r.render_rays(depth, spp, o, d, flat, pixel_base=row * W + col0, want_linear=True)
    print(prec, defocus, "pixels differing:", int((lin != lin_w).any(1).sum()), "segments", st.ray_segments, st_w.ray_segments)
    assert code == rc_w
    assert_same(lin, lin_w, "linear")
    assert np.array_equal(rgb, rgb_w)
    assert st.ray_segments == st_w.ray_segments and st.bounce_iters == st_w.bounce_iters and st.samples == st_w.samples
    assert (lin_w != lin_w[0]).any() and st.ray_segments > ncol * spp, "the segment crosses spheres"


# ---------------------------------------------------------------- 3. per-sample rays, reference B
@pytest.mark.parametrize("R", (2, 3, 7))
@pytest.mark.parametrize("prec", rc.PRECS)
def test_per_sample_rays_against_the_restatement(renderers, prec, R):
    flat = rc.scene("s100")
    o, d = rc.per_sample_rays(prec, R)
    rgb_b, lin_b, segs_b, rc_b = rc.reference_b(flat, o, d, 7, 6, prec)
    rgb, lin, st, code = renderers[prec].render_rays(6, 7, o, d, flat, pixel_base=BASE, want_linear=True)
    print(prec, R, "pixels differing:", int((lin != lin_b).any(1).sum()), "segments", st.ray_segments, segs_b)
    assert code == rc_b
    assert_same(lin, lin_b, "linear")
    assert np.array_equal(rgb, rgb_b)
    assert st.ray_segments == segs_b and st.samples == 12 * 7


def three_ray_pixels(prec):
    """130 pixels of 3 rays: the single-ray set and two neighbours of each ray."""
    o, tgt, _ = rc.ray_set(prec)
    T = rc.DTYPES[prec]
    off = np.array([[0.0, 0.0, 0.0], [0.03, 0.0, -0.02], [-0.02, 0.01, 0.03]])
    t3 = (tgt[:, None, :].astype(np.float64) + off[None]).astype(T)
    o3 = np.repeat(o[:, None, :], 3, 1)
    d3 = np.stack([rc.unit_dirs(o3[:, k], t3[:, k]) for k in range(3)], 1)
    return np.ascontiguousarray(o3), np.ascontiguousarray(d3)


# ---------------------------------------------------------------- 4. invalid rays
@pytest.mark.parametrize("prec", rc.PRECS)
def test_invalid_rays_blank_their_pixels_only(renderers, prec):
    flat = rc.scene("s100")
    o, d = three_ray_pixels(prec)
    r = renderers[prec]
    rgb_w, lin_w, st_w, rc_w = r.render_rays(8, 7, o, d, flat, pixel_base=BASE, want_linear=True)
    o2, d2 = o.copy(), d.copy()
    d2[5, 1, 2] = np.nan
    o2[64, 0, 0] = np.inf
    d2[129, 2] = 0.0
    bad = np.zeros(rc.N_PIX, bool)
    bad[[5, 64, 129]] = True
    rgb, lin, st, code = r.render_rays(8, 7, o2, d2, flat, pixel_base=BASE, want_linear=True)
    assert np.isnan(lin[bad]).all() and (rgb[bad] == 0).all()
    assert_same(lin[~bad], lin_w[~bad], "the other pixels")
    assert np.array_equal(rgb[~bad], rgb_w[~bad]) and np.isfinite(lin_w).all()
    assert st.pixels == rc.N_PIX and st.samples == (rc.N_PIX - 3) * 7 and st_w.samples == rc.N_PIX * 7
    assert st.ray_segments < st_w.ray_segments
    if rc_w == abi.RT_OK:
        assert code == abi.RT_OK, "an invalid pixel raises no RT_ERR_RANGE"
    # every pixel invalid: nothing is traced
    rgb, lin, st, code = r.render_rays(8, 7, o2[bad], d2[bad], flat, want_linear=True)
    assert np.isnan(lin).all() and (rgb == 0).all() and code == abi.RT_OK and st.samples == 0 and st.ray_segments == 0


# ---------------------------------------------------------------- 5. origin forms
@pytest.mark.parametrize("prec", rc.PRECS)
def test_shared_origin_equals_per_ray_copies(renderers, prec):
    flat = rc.scene("s100")
    _, d = three_ray_pixels(prec)
    origin = np.array([13.0, 2.0, 3.1])   # 3.1 is not a float32: the library rounds it as (T)origin[i]
    copies = np.broadcast_to(origin.astype(rc.DTYPES[prec]), d.shape)
    r = renderers[prec]
    rgb_s, lin_s, st_s, rc_s = r.render_rays(8, 6, origin, d, flat, pixel_base=BASE, want_linear=True)
    rgb_c, lin_c, st_c, rc_c = r.render_rays(8, 6, copies, d, flat, pixel_base=BASE, want_linear=True)
    assert rc_s == rc_c
    assert_same(lin_s, lin_c, "linear")
    assert np.array_equal(rgb_s, rgb_c) and st_s.ray_segments == st_c.ray_segments > rc.N_PIX * 6
    assert st_s.kernel_id == st_c.kernel_id and not abi.kernel_info(st_s.kernel_id)["camq"]


# ---------------------------------------------------------------- 6. launch-shape independence
@pytest.mark.parametrize("prec", rc.PRECS)
def test_a_pixel_does_not_depend_on_the_launch(renderers, prec):
    flat = rc.scene("s100")
    o, d = three_ray_pixels(prec)
    r = renderers[prec]
    rgb_w, lin_w, _, _ = r.render_rays(8, 7, o, d, flat, pixel_base=BASE, want_linear=True)
    for p in range(rc.N_PIX):
        rgb, lin, st, _ = r.render_rays(8, 7, o[p:p + 1], d[p:p + 1], flat, pixel_base=BASE + p, want_linear=True)
        assert_same(lin[0], lin_w[p], f"pixel {p}")
        assert np.array_equal(rgb[0], rgb_w[p]) and st.pixels == 1 and st.samples == 7


# ---------------------------------------------------------------- 7. RT_ERR_RANGE
@pytest.mark.parametrize("prec", rc.PRECS)
def test_range_error_comes_back_with_the_image(renderers, prec):
    hot = rt.FlatScene(np.array([[0.0, 0.0, 0.0]]), np.array([5.0]), np.array([0], np.uint32), [rt.Lambertian((9.0, 9.0, 9.0))])
    o, tgt, d = rc.ray_set(prec)
    o = (o.astype(np.float64) + np.array([0.0, 8.0, 0.0])).astype(rc.DTYPES[prec])   # above the sphere, looking down at it
    d = rc.unit_dirs(o, tgt)
    rgb_a, lin_a, segs_a, rc_a = rc.reference_a(hot, o, tgt, 8, 4, prec)
    assert rc_a == abi.RT_ERR_RANGE and (lin_a > 2.0).any()
    rgb, lin, st, code = renderers[prec].render_rays(4, 8, o, d, hot, pixel_base=BASE, want_linear=True)
    assert code == abi.RT_ERR_RANGE
    assert_same(lin, lin_a, "linear")
    assert np.array_equal(rgb, rgb_a) and st.ray_segments == segs_a


# ---------------------------------------------------------------- 8. the kernel id across calls
def test_kernel_id_follows_the_last_call(renderers):
    flat = rc.scene("s100")
    o, _, d = rc.ray_set("f64")
    r = renderers["f64"]
    r.query(o, d, flat)
    assert abi.RT_KERNEL_QUERY(r.query_stats.kernel_id) and not abi.RT_KERNEL_RAYS(r.query_stats.kernel_id)
    _, _, st, _ = r.render_rays(2, 2, o, d, flat)
    assert abi.RT_KERNEL_RAYS(st.kernel_id) and not abi.RT_KERNEL_QUERY(st.kernel_id) and not abi.RT_KERNEL_GUIDES(st.kernel_id)
    cam = rt.camera_new_py(16, 9, **rt.MAIN_CAMERA)
    _, _, st, _ = r.render_flat(2, 2, flat, cam)
    assert not abi.RT_KERNEL_RAYS(st.kernel_id)
    rgb, lin, st, code = r.render_rays(2, 2, o[:0], d[:0], flat, want_linear=True)   # no pixels: nothing is enqueued
    assert rgb.shape == lin.shape == (0, 3) and st.kernel_id == 0 and code == abi.RT_OK


# ---------------------------------------------------------------- 9. torch
@pytest.mark.parametrize("prec", rc.PRECS)
def test_render_rays_into_with_torch_tensors(prec):
    """Torch device tensors, in place, on a non-default torch stream: the values of render_rays() with numpy.  In a
    process of its own (tests/render_rays_into_child.py), for the reason tests/query_into_child.py gives."""
    run = subprocess.run([sys.executable, os.path.join(HERE, "render_rays_into_child.py"), prec], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0 and "render_rays_into ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


# ---------------------------------------------------------------- 10, 11. rt-render --projection
FROM = (16.0, 2.0, 18.5)   # the CLI's default camera (main.rs:51-58)


@pytest.mark.parametrize("prec", rc.PRECS)
@pytest.mark.parametrize("model", ("ortho", "equirect", "fisheye"))
def test_cli_projection(tmp_path, renderers, model, prec):
    from PIL import Image
    W, H, G, spp, depth = 16, 9, 2, 6, 8
    scene = rt.scenes.three_spheres()
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(scene))
    o, d = rt.projections.camera_rays(model, W, H, FROM, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), grid=G, precision=prec,
                                      angle_deg=150.0, extent=7.0)
    rgb, lin, st, code = renderers[prec].render_rays(depth, spp, o, d, scene.flatten(), want_linear=True)
    assert code == abi.RT_OK and (rgb.max(1) > 0).sum() > W * H // 4
    if model == "fisheye":
        out = (d == 0).all(-1).any(1)
        assert out.any() and (rgb[out] == 0).all() and np.isnan(lin[out]).all() and (rgb[~out].max(1) > 0).mean() > 0.9
        assert out.reshape(H, W)[:, 0].all() and not out.reshape(H, W)[:, W // 2].any(), "black outside the circle"
    args = [CLI, "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(depth), "--projection", model,
            "--aa", str(G), "--proj-angle", "150", "--proj-extent", "7"] + (["--f32"] if prec == "f32" else [])
    for out_name in ("o.png", "o.ppm"):
        run = subprocess.run(args + ["--out", out_name], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        assert f"Image Size: {W} x {H}" in run.stdout and f"Total Pixels: {W * H}" in run.stdout
    img = np.asarray(Image.open(tmp_path / "o.png").convert("RGB"))
    assert np.array_equal(img.reshape(-1, 3), rgb)
    raw = (tmp_path / "o.ppm").read_bytes()
    assert raw.startswith(b"P6") and raw[-W * H * 3:] == rgb.tobytes()
    if model == "ortho" and prec == "f64":   # the options that do not go with it, each with a message
        for extra in (["--mode", "scalar"], ["--block-size", "8"], ["--sample-parallel"], ["--progressive", "2"],
                      ["--adaptive", "0.1", "--spp-min", "2"], ["--guides"], ["--pick", "1,1"], ["--aa", "3"]):
            bad = subprocess.run(args + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
            assert bad.returncode == 2 and "--projection" in bad.stderr, (extra, bad.stderr)
