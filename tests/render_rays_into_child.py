"""GpuRenderer.render_rays_into with torch ROCm tensors on a non-default torch stream, against GpuRenderer.render_rays
with numpy.  Run by tests/test_gpu_ray_render.py in a process of its own:

    python tests/render_rays_into_child.py f32|f64

torch has to be imported before rt_mi355x loads its library (tests/query_into_child.py has the reason).  Prints
"render_rays_into ok" and exits 0, or fails an assertion.
"""
import ctypes
import os
import sys

import torch   # first: see above

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "rust-ray-tracing_amd"), HERE):
    sys.path.insert(0, os.path.abspath(p))

import numpy as np   # noqa: E402
import rt_mi355x as rt   # noqa: E402
from rt_mi355x import abi   # noqa: E402


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)
    if got.dtype.kind == "f":   # 0 ulp: NaN patterns and signed zeros too
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64),
                                      err_msg=what)


def main(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    n, R, spp, depth, base = 200, 2, 5, 8, 4096
    rng = np.random.default_rng(11)
    flat = rt.scenes.random_spheres(100).flatten()
    P = np.array(rt.MAIN_CAMERA["center"])
    o = (P + rng.uniform(-3, 3, (n, R, 3))).astype(dtype)
    d = (-P / np.linalg.norm(P) + 0.3 * rng.standard_normal((n, R, 3))).astype(dtype)
    d[5, 1] = np.nan   # an invalid ray: its pixel comes back NaN / black
    r = rt.GpuRenderer(precision=prec)
    try:
        rgb_g, lin_g, st_g, rc_g = r.render_rays(depth, spp, o, d, flat, pixel_base=base, want_linear=True)
        rgb_s, lin_s, _, rc_s = r.render_rays(depth, spp, P, d, flat, pixel_base=base, want_linear=True)
        assert np.isnan(lin_g[5]).all() and np.isfinite(np.delete(lin_g, 5, 0)).all() and st_g.samples == (n - 1) * spp
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        with torch.cuda.stream(stream):
            d_t, o_t = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
            rgb_t = torch.full((n, 3), 7, dtype=torch.uint8, device=dev)
            lin_t = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev)
            for origins, rgb_w, lin_w, rc_w in ((o_t, rgb_g, lin_g, rc_g), (tuple(float(x) for x in P), rgb_s, lin_s, rc_s)):
                assert r.render_rays_into(depth, spp, origins, d_t, rgb=rgb_t, linear=lin_t, pixel_base=base,
                                          stream=stream.cuda_stream) == n
                stream.synchronize()
                same(lin_t.cpu().numpy(), lin_w, "linear")
                same(rgb_t.cpu().numpy(), rgb_w, "rgb")
                st = abi.RtStats()
                rc = r.lib.rt_context_collect(r.ctx, ctypes.c_void_p(stream.cuda_stream), ctypes.byref(st))
                assert rc == rc_w and st.pixels == n and st.samples == (n - 1) * spp and abi.RT_KERNEL_RAYS(st.kernel_id)
                rgb_t.fill_(7)
                lin_t.fill_(7)
            # in place, no copy: only the output that was given is written; (n, 3) directions are one ray per pixel
            assert r.render_rays_into(depth, spp, o_t[:, 0].contiguous(), d_t[:, 0].contiguous(), linear=lin_t,
                                      pixel_base=base, stream=stream.cuda_stream) == n
            stream.synchronize()
            _, lin_1, _, _ = r.render_rays(depth, spp, o[:, 0], d[:, 0], flat, pixel_base=base, want_linear=True)
            same(lin_t.cpu().numpy(), lin_1, "linear, R = 1")
            assert (rgb_t == 7).all().item()
            r.lib.rt_context_collect(r.ctx, ctypes.c_void_p(stream.cuda_stream), None)
            for bad, exc, kw in ((d_t.to(torch.float16), ValueError, dict(rgb=rgb_t)),
                                 (d_t, ValueError, dict(linear=torch.zeros((3, n), dtype=torch.float64, device=dev).T)),
                                 (d_t, ValueError, dict(rgb=lin_t)),
                                 (d_t.cpu(), TypeError, dict(rgb=rgb_t))):
                try:
                    r.render_rays_into(depth, spp, o_t, bad, **kw)
                except exc:
                    continue
                raise AssertionError(f"render_rays_into accepted {tuple(bad.shape)} {bad.dtype} {bad.device} with {sorted(kw)}")
    finally:
        r.close()
    print("render_rays_into ok")


if __name__ == "__main__":
    main(sys.argv[1])
