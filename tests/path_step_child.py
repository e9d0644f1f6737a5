"""GpuRenderer.path_step_into and scatter_into with torch ROCm tensors on a non-default torch stream, against
GpuRenderer.path_step and scatter with numpy.  Run by tests/test_gpu_path_step.py in a process of its own:

    python tests/path_step_child.py f32|f64

torch carries a HIP runtime of its own, and a process can hold one: torch has to be imported before rt_mi355x loads
its library (tests/query_into_child.py has the whole story).  Prints "path_step_into ok" and exits 0, or fails an
assertion.
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

SEED = 0xDEADBEEF5EED0001


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)
    if got.dtype.kind == "f":   # 0 ulp: NaN and inf patterns and signed zeros too
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u), err_msg=what)


def collect(r, stream):
    st = abi.RtStats()
    abi.check(r.lib, r.lib.rt_context_collect(r.ctx, ctypes.c_void_p(stream.cuda_stream), ctypes.byref(st)))
    return st


def main(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    tt = torch.float32 if prec == "f32" else torch.float64
    n = 1000
    rng = np.random.default_rng(11)
    flat = rt.scenes.random_spheres(100).flatten()
    P = np.array(rt.MAIN_CAMERA["center"])
    o = (P + rng.uniform(-6, 6, (n, 3))).astype(dtype)
    d = (-P / np.linalg.norm(P) + 0.4 * rng.standard_normal((n, 3))).astype(dtype)
    d[5] = np.nan   # an invalid ray among them
    pix = rng.integers(0, 1 << 20, n).astype(np.uint32)
    smp = rng.integers(0, 64, n).astype(np.uint32)
    col = rng.uniform(0.1, 1.0, (n, 3)).astype(dtype)
    r = rt.GpuRenderer(precision=prec, seed=SEED)
    try:
        want = r.path_step(o, d, flat, pixel=pix, sample=smp, bounce=2, colour=col, root2=True)
        hits = want["status"] == abi.RT_STEP_SCATTERED
        assert hits.mean() > 0.2 and (want["status"] == abi.RT_STEP_MISSED).any() and want["status"][5] == abi.RT_STEP_INVALID
        want_s = r.scatter(o, d, want["index"], want["t"], flat, pixel=pix, sample=smp, bounce=2, colour=col)
        for key in ("origins", "directions", "colour"):
            same(want_s[key], want[key], f"scatter after query: {key}")
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        T = lambda a: torch.from_numpy(a.copy()).to(dev)   # noqa: E731
        with torch.cuda.stream(stream):
            o_t, d_t, c_t, pix_t, smp_t = T(o), T(d), T(col), T(pix.view(np.int32)).view(torch.uint32), T(smp.view(np.int32)).view(torch.uint32)
            outs = dict(status=torch.full((n,), 7, dtype=torch.uint8, device=dev), index=torch.full((n,), 7, dtype=torch.int32, device=dev),
                        t=torch.full((n,), 7.0, dtype=tt, device=dev), normal=torch.full((n, 3), 7.0, dtype=tt, device=dev),
                        front=torch.full((n,), 7, dtype=torch.uint8, device=dev))
            assert r.path_step_into(o_t, d_t, pix_t, smp_t, bounce=2, colour=c_t, stream=stream.cuda_stream, root2=True, **outs) == n
            stream.synchronize()
            for key in ("status", "index", "t", "normal", "front"):
                same(outs[key].cpu().numpy(), want[key], key)
            for key, ten in (("origins", o_t), ("directions", d_t), ("colour", c_t)):
                same(ten.cpu().numpy(), want[key], key)
            st = collect(r, stream)
            assert st.pixels == n and st.samples == n - 1 and st.ray_segments == n - 1 and abi.RT_KERNEL_STEP(st.kernel_id)
            # in place, no copy: only the outputs that were given are written; no colour tracked
            o_t, d_t = T(o), T(d)
            for v in outs.values():
                v.fill_(7)
            assert r.path_step_into(o_t, d_t, pix_t, smp_t, bounce=2, stream=stream.cuda_stream, root2=True,
                                    status=outs["status"], t=outs["t"]) == n
            stream.synchronize()
            same(outs["status"].cpu().numpy(), want["status"], "status")
            same(outs["t"].cpu().numpy(), want["t"], "t")
            same(d_t.cpu().numpy(), want["directions"], "directions")
            assert (outs["normal"] == 7).all().item() and (outs["index"] == 7).all().item() and (outs["front"] == 7).all().item()
            collect(r, stream)
            # scatter_into: a query's index and t on the device, separate outputs and in place
            o_t, d_t, c_t = T(o), T(d), T(col)
            i_t, t_t = T(want["index"]), T(want["t"])
            oo, od = torch.zeros((n, 3), dtype=tt, device=dev), torch.zeros((n, 3), dtype=tt, device=dev)
            assert r.scatter_into(o_t, d_t, i_t, t_t, pix_t, smp_t, bounce=2, colour=c_t, out_origins=oo, out_directions=od,
                                  stream=stream.cuda_stream) == n
            stream.synchronize()
            same(oo.cpu().numpy(), want["origins"], "scatter_into origins")
            same(od.cpu().numpy(), want["directions"], "scatter_into directions")
            same(c_t.cpu().numpy(), want["colour"], "scatter_into colour")
            same(d_t.cpu().numpy(), d, "the inputs stay")
            st = collect(r, stream)
            assert st.samples == int(hits.sum()) and st.ray_segments == 0 and abi.RT_KERNEL_SCATTER(st.kernel_id)
            assert r.scatter_into(o_t, d_t, i_t, t_t, pix_t, smp_t, bounce=2, stream=stream.cuda_stream) == n
            stream.synchronize()
            same(o_t.cpu().numpy(), want["origins"], "in place origins")
            same(d_t.cpu().numpy(), want["directions"], "in place directions")
            collect(r, stream)
            for bad, exc in ((dict(directions=d_t.to(torch.float16)), ValueError), (dict(pixel=pix_t.view(torch.int32)), ValueError),
                             (dict(directions=d_t.cpu()), TypeError), (dict(origins=o_t.T.contiguous().T), ValueError)):
                args = dict(origins=o_t, directions=d_t, pixel=pix_t, sample=smp_t)
                args.update(bad)
                try:
                    r.path_step_into(args["origins"], args["directions"], args["pixel"], args["sample"])
                except exc:
                    continue
                raise AssertionError(f"path_step_into accepted {sorted(bad)}")
    finally:
        r.close()
    print("path_step_into ok")


if __name__ == "__main__":
    main(sys.argv[1])
