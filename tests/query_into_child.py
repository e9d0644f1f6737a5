"""GpuRenderer.query_into with torch ROCm tensors on a non-default torch stream, against GpuRenderer.query with numpy.
Run by tests/test_gpu_query.py in a process of its own:

    python tests/query_into_child.py f32|f64

torch carries a HIP runtime of its own, and a process can hold one: torch has to be imported before rt_mi355x loads
its library, which then binds to the runtime torch brought.  The test session loaded the library long before, hence
the child process.  Prints "query_into ok" and exits 0, or fails an assertion.
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

ALL = ("t", "index", "normal", "point", "front")


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)
    if got.dtype.kind == "f":   # 0 ulp: NaN and inf patterns and signed zeros too
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u), err_msg=what)


def main(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    tt = torch.float32 if prec == "f32" else torch.float64
    n = 1000
    rng = np.random.default_rng(7)
    flat = rt.scenes.random_spheres(100).flatten()
    P = np.array(rt.MAIN_CAMERA["center"])
    o = (P + rng.uniform(-6, 6, (n, 3))).astype(dtype)
    d = (-P / np.linalg.norm(P) + 0.4 * rng.standard_normal((n, 3))).astype(dtype)
    d[5] = np.nan   # an invalid ray among them
    r = rt.GpuRenderer(precision=prec)
    try:
        want_g = r.query(o, d, flat, root2=True)
        want_s = r.query(P, d, flat, root2=True)
        assert (want_g["index"] >= 0).mean() > 0.2 and (want_g["index"] == -1).any() and want_g["index"][5] == -2
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        with torch.cuda.stream(stream):
            d_t, o_t = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
            outs = dict(t=torch.full((n,), 7.0, dtype=tt, device=dev), index=torch.full((n,), 7, dtype=torch.int32, device=dev),
                        normal=torch.full((n, 3), 7.0, dtype=tt, device=dev), point=torch.full((n, 3), 7.0, dtype=tt, device=dev),
                        front=torch.full((n,), 7, dtype=torch.uint8, device=dev))
            for origins, want in ((o_t, want_g), (tuple(float(x) for x in P), want_s)):
                assert r.query_into(origins, d_t, stream=stream.cuda_stream, root2=True, **outs) == n
                stream.synchronize()
                for key in ALL:
                    same(outs[key].cpu().numpy(), want[key], key)
                st = abi.RtStats()
                abi.check(r.lib, r.lib.rt_context_collect(r.ctx, ctypes.c_void_p(stream.cuda_stream), ctypes.byref(st)))
                assert st.pixels == n and st.samples == n - 1 and abi.RT_KERNEL_QUERY(st.kernel_id)
                assert abi.kernel_info(st.kernel_id)["camq"] is isinstance(origins, tuple)
                for v in outs.values():
                    v.fill_(7)
            # in place, no copy: only the outputs that were given are written
            part = dict(outs, normal=None, front=None)
            assert r.query_into(o_t, d_t, stream=stream.cuda_stream, root2=True, **part) == n
            stream.synchronize()
            same(outs["t"].cpu().numpy(), want_g["t"], "t")
            same(outs["point"].cpu().numpy(), want_g["point"], "point")
            assert (outs["normal"] == 7).all().item() and (outs["front"] == 7).all().item()
            abi.check(r.lib, r.lib.rt_context_collect(r.ctx, ctypes.c_void_p(stream.cuda_stream), None))
            for bad, exc, kw in ((d_t.to(torch.float16), ValueError, dict(t=outs["t"])),
                                 (d_t, ValueError, dict(point=torch.zeros((3, n), dtype=tt, device=dev).T)),
                                 (d_t, ValueError, dict(index=outs["front"])),
                                 (d_t.cpu(), TypeError, dict(t=outs["t"]))):
                try:
                    r.query_into(o_t, bad, **kw)
                except exc:
                    continue
                raise AssertionError(f"query_into accepted {tuple(bad.shape)} {bad.dtype} {bad.device} with {sorted(kw)}")
    finally:
        r.close()
    print("query_into ok")


if __name__ == "__main__":
    main(sys.argv[1])
