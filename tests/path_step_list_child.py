"""GpuRenderer.path_step_list_into and compact_list_into with torch ROCm tensors on a non-default torch stream: two
steps chained through the device count with no host read between them, against GpuRenderer.path_step with numpy.  Run
by tests/test_gpu_ray_list.py in a process of its own:

    python tests/path_step_list_child.py f32|f64

torch has to be imported before rt_mi355x loads its library (tests/query_into_child.py has the whole story).  Prints
"path_step_list_into ok" and exits 0, or fails an assertion.
"""
import os
import sys

import torch   # first: see above

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "rust-ray-tracing_amd"), HERE):
    sys.path.insert(0, os.path.abspath(p))

import numpy as np   # noqa: E402
import rt_mi355x as rt   # noqa: E402
from path_step_child import SEED, collect, same   # noqa: E402
from rt_mi355x import abi   # noqa: E402


def main(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    n = 1000
    rng = np.random.default_rng(12)
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
        # the expectation, with numpy: step 0 over every ray, step 1 over the rays step 0 scattered
        s0 = r.path_step(o, d, flat, pixel=pix, sample=smp, bounce=0, colour=col)
        live0 = np.flatnonzero(s0["status"] == abi.RT_STEP_SCATTERED).astype(np.uint32)
        assert 100 < live0.size < n and s0["status"][5] == abi.RT_STEP_INVALID
        s1 = r.path_step(s0["origins"], s0["directions"], flat, pixel=pix, sample=smp, bounce=1, colour=s0["colour"])
        want = {k: s0[k].copy() for k in ("origins", "directions", "colour", "status")}
        for k in want:
            want[k][live0] = s1[k][live0]
        live1 = live0[s1["status"][live0] == abi.RT_STEP_SCATTERED]
        assert 0 < live1.size < live0.size

        dev = torch.device("cuda", r.device)
        stream = torch.cuda.Stream(device=dev)
        assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        T = lambda a: torch.from_numpy(a.copy()).to(dev)   # noqa: E731
        U = lambda a: T(a.view(np.int32)).view(torch.uint32)   # noqa: E731
        word = np.uint32(0xDEADBEEF)
        H = lambda ten: ten.view(torch.int32).cpu().numpy().view(np.uint32)   # noqa: E731
        with torch.cuda.stream(stream):
            o_t, d_t, c_t, pix_t, smp_t = T(o), T(d), T(col), U(pix), U(smp)
            status = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            lists = [U(np.full(n, word, np.uint32)) for _ in range(2)]
            counts = [U(np.full(1, word, np.uint32)) for _ in range(2)]
            kw = dict(colour=c_t, status=status, stream=stream.cuda_stream)
            assert r.path_step_list_into(o_t, d_t, pix_t, smp_t, bounce=0, list_out=lists[0], count_out=counts[0], **kw) == n
            assert r.path_step_list_into(o_t, d_t, pix_t, smp_t, bounce=1, list_in=lists[0], count_in=counts[0],
                                         list_out=lists[1], count_out=counts[1], **kw) == n   # no host read in between
            # and a list from the final status array: the rays that were not missed
            assert r.compact_list_into(status, lists[0], counts[0], stream=stream.cuda_stream) == n
            stream.synchronize()
            for key, ten in (("origins", o_t), ("directions", d_t), ("colour", c_t), ("status", status)):
                same(ten.cpu().numpy(), want[key], key)
            got = H(lists[1])
            k = int(H(counts[1])[0])
            assert k == live1.size
            same(got[:k], live1, "the list after two steps")
            assert (got[k:] == word).all()
            kept = np.flatnonzero(want["status"] != abi.RT_STEP_MISSED).astype(np.uint32)
            k = int(H(counts[0])[0])
            assert k == kept.size and 5 in kept
            same(H(lists[0])[:k], kept, "the list from the status array")
            st = collect(r, stream)
            valid = (n - 1) + int((s1["status"][live0] != abi.RT_STEP_INVALID).sum())
            assert st.pixels == 3 * n and st.samples == valid and st.ray_segments == valid
            assert abi.RT_KERNEL_LIST(st.kernel_id) and abi.RT_KERNEL_STEP(st.kernel_id)
            for bad, exc in ((dict(list_in=lists[0].view(torch.int32)), ValueError), (dict(list_in=lists[0].cpu()), TypeError),
                             (dict(list_out=lists[0]), ValueError), (dict(list_in=lists[0], list_out=lists[0], count_out=counts[0]), ValueError),
                             (dict(count_in=counts[0], list_out=lists[1], count_out=counts[0]), ValueError)):
                try:
                    r.path_step_list_into(o_t, d_t, pix_t, smp_t, bounce=2, **bad)
                except exc:
                    continue
                raise AssertionError(f"path_step_list_into accepted {sorted(bad)}")
    finally:
        r.close()
    print("path_step_list_into ok")


if __name__ == "__main__":
    main(sys.argv[1])
