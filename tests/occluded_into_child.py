"""GpuRenderer.occluded_into with torch ROCm tensors on a non-default torch stream, against GpuRenderer.occluded with
numpy.  Run by tests/test_gpu_occlusion.py in a process of its own, for tests/query_into_child.py's reason (torch has
to be imported before rt_mi355x loads its library):

    python tests/occluded_into_child.py f32|f64

Prints "occluded_into ok" and exits 0, or fails an assertion.
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


def main(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    n = 1000
    rng = np.random.default_rng(7)
    flat = rt.scenes.random_spheres(100).flatten()
    P = np.array(rt.MAIN_CAMERA["center"])
    o = (P + rng.uniform(-6, 6, (n, 3))).astype(dtype)
    d = (-P / np.linalg.norm(P) + 0.4 * rng.standard_normal((n, 3))).astype(dtype)
    d[5] = np.nan   # an invalid ray among them
    r = rt.GpuRenderer(precision=prec)
    try:
        t = r.query(o, d, flat, root2=True, want=("t",))["t"]
        bound = float(np.median(t[np.isfinite(t)]))
        tm = np.where(np.arange(n) % 2 == 0, dtype(bound), dtype(np.inf)).astype(dtype)
        tm[9] = np.nan
        want = {"array_g": r.occluded(o, d, flat, t_max=tm, root2=True), "scalar_g": r.occluded(o, d, flat, t_max=bound, root2=True),
                "array_s": r.occluded(P, d, flat, t_max=tm, root2=True), "scalar_s": r.occluded(P, d, flat, t_max=bound, root2=True)}
        for w in want.values():
            assert w[5] == 255 and (w == 1).mean() > 0.1 and (w == 0).mean() > 0.1
        assert want["array_g"][9] == 255 and want["scalar_g"][9] != 255
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(want["array_g"], np.where(np.isnan(t) | np.isnan(tm), 255, t < tm).astype(np.uint8))
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        with torch.cuda.stream(stream):
            d_t, o_t, tm_t = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(tm).to(dev)
            out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            for origins, path in ((o_t, "g"), (tuple(float(x) for x in P), "s")):
                for bound_arg, form in ((tm_t, "array"), (bound, "scalar")):
                    assert r.occluded_into(origins, d_t, out, t_max=bound_arg, stream=stream.cuda_stream, root2=True) == n
                    stream.synchronize()
                    np.testing.assert_array_equal(out.cpu().numpy(), want[f"{form}_{path}"], err_msg=f"{form} {path}")
                    st = abi.RtStats()
                    abi.check(r.lib, r.lib.rt_context_collect(r.ctx, ctypes.c_void_p(stream.cuda_stream), ctypes.byref(st)))
                    assert st.pixels == n and st.samples == n - (2 if form == "array" else 1)
                    assert abi.RT_KERNEL_OCCLUSION(st.kernel_id) and not abi.kernel_info(st.kernel_id)["camq"]
                    out.fill_(7)
            for bad_d, bad_out, bad_t, exc in ((d_t.to(torch.float16), out, 1.0, ValueError),
                                               (d_t, out.to(torch.int32), 1.0, ValueError),
                                               (d_t, out, tm_t[:-1], ValueError),
                                               (d_t, out, tm_t.cpu(), TypeError),
                                               (d_t.cpu(), out, 1.0, TypeError)):
                try:
                    r.occluded_into(o_t, bad_d, bad_out, t_max=bad_t)
                except exc:
                    continue
                raise AssertionError("occluded_into accepted a bad argument")
    finally:
        r.close()
    print("occluded_into ok")


if __name__ == "__main__":
    main(sys.argv[1])
