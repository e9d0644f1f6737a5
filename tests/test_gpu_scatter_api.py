"""rt_scatter_async on the device (scatter_rays<T>) against the oracle's next-ray probe.  Bar: 0 ulp everywhere; every
comparison is query_cases.assert_same (the values and the bit patterns, NaN patterns and signed zeros included).

  * every lane of the ten families of tests/scatter_cases.py (tests/step_cases.py lays them out; tests/test_step_cases.py
    checks that layout on the CPU): the front bit at a zero dot, TIR and Schlick one ulp either side, near-zero
    Lambertian sums, subnormal colours, signed and tiny radii, mixed waves.  A call has one bounce, so a family runs
    as one call per bounce its lanes use, in place on the same device arrays: a lane is a hit in the call of its own
    bounce and a miss (-1) or an invalid ray (-2) in every other, so each call must also hand back, bit for bit, what
    the calls before it left;
  * n = 1, 63, 64, 65 and 300 with lanes of index -1 and -2 interleaved: in place against separate outputs, both
    origin forms, d_colour NULL, both precisions;
  * an index >= n_spheres and a sample >= 2^20: RT_ERR_INVALID at the collect, the other lanes untouched by it.
"""
import ctypes

import numpy as np
import pytest

import oracle_bind as ob
import scatter_cases as sc
import step_cases as stc
from query_cases import assert_same
from rt_mi355x import abi
from rt_mi355x.integrators import DeviceArray

pytestmark = pytest.mark.gpu

F32 = abi.RT_FLAG_F32


@pytest.fixture(autouse=True)
def _leave_the_shared_renderer_as_it_was(renderer):
    flags, seed = renderer.flags, renderer.seed
    yield
    renderer.flags, renderer.seed = flags, seed


def setup(renderer, prec):
    renderer.flags = F32 if prec == "f32" else 0
    renderer.seed = sc.SEED
    renderer._use_scene(sc.table())


def collect(renderer, want=abi.RT_OK):
    st = abi.RtStats()
    rc = renderer.lib.rt_context_collect(renderer.ctx, None, ctypes.byref(st))
    assert rc == want, (rc, renderer.lib.rt_last_error())
    return st


def check_scatter_stats(st, prec, n, scattered):
    assert st.pixels == n and st.samples == scattered and st.ray_segments == 0 and st.bounce_iters == 0
    assert st.lane_slots == 0 and st.box_groups == 0 and st.exact_tests == 0
    k = abi.kernel_info(st.kernel_id)
    assert abi.RT_KERNEL_SCATTER(st.kernel_id) == 1 and k["scatter"] and not k["step"] and not k["query"]
    assert abi.kernel_name(st.kernel_id) == f"scatter_rays<{'float' if prec == 'f32' else 'double'}>"


# ---------------------------------------------------------------- 1. the ten families
@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_families(renderer, family, prec):
    la = stc.family_lanes(family, prec)
    setup(renderer, prec)
    go = la.index >= 0
    bounces = np.unique(la.k[go])
    lane = np.arange(la.n)
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        d_o, d_d, d_c = DeviceArray(dev, la.o), DeviceArray(dev, la.d), DeviceArray(dev, la.c)
        d_t, d_pix, d_smp = DeviceArray(dev, la.t), DeviceArray(dev, la.pixel), DeviceArray(dev, la.sample)
        d_idx = DeviceArray(dev, shape=(la.n,), dtype=np.int32)
        if bounces.size == 0:   # the camera family: every lane a miss
            bounces = np.array([0], np.uint32)
        for k in bounces:
            mine = go & (la.k == k)
            d_idx.set(np.where(mine, la.index, np.where(lane % 2 == 0, abi.RT_QUERY_MISS, abi.RT_QUERY_INVALID)).astype(np.int32))
            assert renderer.scatter_into(d_o, d_d, d_idx, d_t, d_pix, d_smp, bounce=int(k), colour=d_c) == la.n
        st = collect(renderer)
        got_o, got_d, got_c = d_o.get(), d_d.get(), d_c.get()
    assert st.pixels == la.n * bounces.size and st.samples == int(go.sum()) and st.ray_segments == 0
    assert abi.RT_KERNEL_SCATTER(st.kernel_id) == 1
    bad = np.flatnonzero((stc.qc.bits(got_o) != stc.qc.bits(la.want_o)).any(1) | (stc.qc.bits(got_d) != stc.qc.bits(la.want_d)).any(1)
                         | (stc.qc.bits(got_c) != stc.qc.bits(la.want_c)).any(1))
    assert bad.size == 0, (f"{family}/{prec}: {bad.size} of {la.n} lanes differ; first lane {bad[0]} (index {la.index[bad[0]]}, "
                           f"bounce {la.k[bad[0]]}): d {got_d[bad[0]].tolist()} want {la.want_d[bad[0]].tolist()}, "
                           f"o {got_o[bad[0]].tolist()} want {la.want_o[bad[0]].tolist()}, "
                           f"c {got_c[bad[0]].tolist()} want {la.want_c[bad[0]].tolist()}")
    assert_same(got_o, la.want_o, "origins")
    assert_same(got_d, la.want_d, "directions")
    assert_same(got_c, la.want_c, "colour")


# ---------------------------------------------------------------- 2. sizes, forms, aliasing
@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("n", stc.SIZES)
def test_sizes_in_place_and_separate(renderer, n, prec):
    la = stc.sized_lanes(prec, n)
    setup(renderer, prec)
    scattered = int((la.index >= 0).sum())
    # numpy in and out: in place on the device
    out = renderer.scatter(la.o, la.d, la.index, la.t, sc.table(), pixel=la.pixel, sample=la.sample, bounce=stc.SIZE_BOUNCE,
                           colour=la.c)
    check_scatter_stats(renderer.query_stats, prec, n, scattered)
    assert_same(out["origins"], la.want_o, "origins, in place")
    assert_same(out["directions"], la.want_d, "directions, in place")
    assert_same(out["colour"], la.want_c, "colour")
    # d_colour NULL: no colour is tracked, the rays are the same
    bare = renderer.scatter(la.o, la.d, la.index, la.t, sc.table(), pixel=la.pixel, sample=la.sample, bounce=stc.SIZE_BOUNCE)
    assert bare["colour"] is None
    assert_same(bare["origins"], la.want_o, "origins without a colour")
    assert_same(bare["directions"], la.want_d, "directions without a colour")
    # separate outputs: the same values, and the inputs stay as they were
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        d_o, d_d, d_c = DeviceArray(dev, la.o), DeviceArray(dev, la.d), DeviceArray(dev, la.c)
        d_idx, d_t = DeviceArray(dev, la.index), DeviceArray(dev, la.t)
        d_pix, d_smp = DeviceArray(dev, la.pixel), DeviceArray(dev, la.sample)
        fill = np.full((n, 3), 7, la.o.dtype)
        o_o, o_d = DeviceArray(dev, fill), DeviceArray(dev, fill)
        renderer.scatter_into(d_o, d_d, d_idx, d_t, d_pix, d_smp, bounce=stc.SIZE_BOUNCE, colour=d_c, out_origins=o_o,
                              out_directions=o_d)
        check_scatter_stats(collect(renderer), prec, n, scattered)
        assert_same(o_o.get(), la.want_o, "origins, separate")
        assert_same(o_d.get(), la.want_d, "directions, separate")
        assert_same(d_c.get(), la.want_c, "colour, separate")
        assert_same(d_o.get(), la.o, "the input origins")
        assert_same(d_d.get(), la.d, "the input directions")
        # one output only (the C entry point: scatter_into's None means in place)
        o_d.set(fill)
        abi.check(renderer.lib, renderer.lib.rt_scatter_async(
            renderer.ctx, n, d_o.ptr, None, d_d.ptr, d_idx.ptr, d_t.ptr, d_pix.ptr, d_smp.ptr, stc.SIZE_BOUNCE, sc.SEED,
            renderer.flags, None, None, o_d.ptr, None))
        collect(renderer)
        assert_same(o_d.get(), la.want_d, "directions alone")
        assert_same(d_o.get(), la.o, "origins not asked for")
        # scatter_into without outputs: in place
        renderer.scatter_into(d_o, d_d, d_idx, d_t, d_pix, d_smp, bounce=stc.SIZE_BOUNCE)
        collect(renderer)
        assert_same(d_o.get(), la.want_o, "origins, in place on the caller's arrays")
        assert_same(d_d.get(), la.want_d, "directions, in place on the caller's arrays")


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("n", [1, 65, 300])
def test_shared_origin(renderer, n, prec):
    """One shared origin (3 host doubles, rounded as a camera centre is): the values of the same rays with that origin
    in every row, and the oracle's."""
    la = stc.sized_lanes(prec, n)
    dtype = stc.DTYPES[prec]
    setup(renderer, prec)
    P = np.array([0.1, 2.0 / 3.0, -1e-3])   # not exact in fp32: the rounding is part of what is compared
    rows = np.ascontiguousarray(np.broadcast_to(P.astype(dtype), (n, 3)))
    shared = renderer.scatter(P, la.d, la.index, la.t, sc.table(), pixel=la.pixel, sample=la.sample, bounce=stc.SIZE_BOUNCE,
                              colour=la.c)
    check_scatter_stats(renderer.query_stats, prec, n, int((la.index >= 0).sum()))
    per_ray = renderer.scatter(rows, la.d, la.index, la.t, sc.table(), pixel=la.pixel, sample=la.sample,
                               bounce=stc.SIZE_BOUNCE, colour=la.c)
    for key in ("origins", "directions", "colour"):
        assert_same(shared[key], per_ray[key], f"{key}: shared origin against per-ray origins")
    go = np.flatnonzero(la.index >= 0)
    want_o, want_d, want_c = rows.copy(), la.d.copy(), la.c.copy()
    if go.size:
        oo, dd, cc, _, _, _ = ob.oracle_next_ray(sc.table(), sc.SEED, "packed", np.ascontiguousarray(rows[go].T),
                                                np.ascontiguousarray(la.d[go].T), la.index[go], la.t[go], la.sample[go],
                                                la.pixel[go], la.k[go], np.ascontiguousarray(la.c[go].T))
        want_o[go], want_d[go], want_c[go] = oo.T, dd.T, cc.T
    assert_same(shared["origins"], want_o, "origins")
    assert_same(shared["directions"], want_d, "directions")
    assert_same(shared["colour"], want_c, "colour")
    # in place with a shared origin: only the directions are written
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        d_d = DeviceArray(dev, la.d)
        renderer.scatter_into(P, d_d, DeviceArray(dev, la.index), DeviceArray(dev, la.t), DeviceArray(dev, la.pixel),
                              DeviceArray(dev, la.sample), bounce=stc.SIZE_BOUNCE)
        collect(renderer)
        assert_same(d_d.get(), want_d, "directions, in place, shared origin")


def test_the_seed_and_the_bounce_key_the_draw(renderer):
    la = stc.sized_lanes("f32", 300)
    setup(renderer, "f32")
    args = dict(pixel=la.pixel, sample=la.sample, colour=la.c)
    base = renderer.scatter(la.o, la.d, la.index, la.t, sc.table(), bounce=stc.SIZE_BOUNCE, **args)
    assert_same(base["directions"], la.want_d, "the renderer's seed")
    other_seed = renderer.scatter(la.o, la.d, la.index, la.t, sc.table(), bounce=stc.SIZE_BOUNCE, seed=sc.SEED ^ 1 << 40, **args)
    other_bounce = renderer.scatter(la.o, la.d, la.index, la.t, sc.table(), bounce=stc.SIZE_BOUNCE + 1, **args)
    go = la.index >= 0
    for other in (other_seed, other_bounce):
        assert (other["directions"][go] != base["directions"][go]).any(1).mean() > 0.5
        assert_same(other["origins"], base["origins"], "the hit point draws nothing")
        assert_same(other["directions"][~go], la.d[~go], "a miss")
    explicit = renderer.scatter(la.o, la.d, la.index, la.t, sc.table(), bounce=stc.SIZE_BOUNCE, seed=sc.SEED, **args)
    assert_same(explicit["directions"], base["directions"], "seed given")


# ---------------------------------------------------------------- 3. lanes outside the contract
@pytest.mark.parametrize("prec", stc.PRECS)
def test_out_of_range_index_and_sample(renderer, prec):
    """index >= n_spheres and sample >= 2^20 (on a lane that would scatter): left as a miss is, RT_ERR_INVALID at the
    collect, the other lanes untouched by it; the next call starts clean."""
    la = stc.sized_lanes(prec, 300)
    n, ns = 130, sc.table().n_spheres
    setup(renderer, prec)
    hits = np.flatnonzero(la.index[:n] >= 0)
    cases = {"index == n_spheres": (hits[3], "index", ns), "index INT32_MAX": (hits[40], "index", 0x7FFFFFFF),
             "sample == 2^20": (hits[21], "sample", 1 << 20), "sample 2^32 - 1": (hits[64], "sample", 0xFFFFFFFF)}
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        d_t, d_pix = DeviceArray(dev, la.t[:n]), DeviceArray(dev, la.pixel[:n])
        for what, (lane, field, value) in cases.items():
            idx, smp = la.index[:n].copy(), la.sample[:n].copy()
            {"index": idx, "sample": smp}[field][lane] = value
            d_o, d_d, d_c = DeviceArray(dev, la.o[:n]), DeviceArray(dev, la.d[:n]), DeviceArray(dev, la.c[:n])
            renderer.scatter_into(d_o, d_d, DeviceArray(dev, idx), d_t, d_pix, DeviceArray(dev, smp), bounce=stc.SIZE_BOUNCE,
                                  colour=d_c)
            st = collect(renderer, abi.RT_ERR_INVALID)
            assert b"rt_scatter_async" in renderer.lib.rt_last_error(), what
            assert st.samples == hits.size - 1 and st.pixels == n, what
            want_o, want_d, want_c = la.want_o[:n].copy(), la.want_d[:n].copy(), la.want_c[:n].copy()
            want_o[lane], want_d[lane], want_c[lane] = la.o[lane], la.d[lane], la.c[lane]
            assert_same(d_o.get(), want_o, f"{what}: origins")
            assert_same(d_d.get(), want_d, f"{what}: directions")
            assert_same(d_c.get(), want_c, f"{what}: colour")
            # a sample >= 2^20 on a lane that is a miss anyway is no error; the flag is per collect
            idx, smp = la.index[:n].copy(), la.sample[:n].copy()
            miss = int(np.flatnonzero(idx < 0)[0])
            smp[miss] = 1 << 20
            d_o, d_d = DeviceArray(dev, la.o[:n]), DeviceArray(dev, la.d[:n])
            renderer.scatter_into(d_o, d_d, DeviceArray(dev, idx), d_t, d_pix, DeviceArray(dev, smp), bounce=stc.SIZE_BOUNCE)
            assert collect(renderer).samples == hits.size
            assert_same(d_d.get(), la.want_d[:n], f"after {what}: a clean call")


def test_refusals_on_a_live_context(renderer, lib):
    import rt_mi355x as rt
    setup(renderer, "f32")
    p = ctypes.c_void_p(16)
    ctx = renderer.ctx
    head = (ctx, 64, p, None, p, p, p, p, p)
    cases = [(head + (0, 7, abi.RT_FLAG_MODE_SCALAR | F32, p, p, p, None), abi.RT_ERR_UNSUPPORTED),
             (head + (0, 7, 0x40, p, p, p, None), abi.RT_ERR_INVALID),
             (head + (0, 7, F32, p, None, None, None), abi.RT_ERR_INVALID),
             (head + (abi.RT_MAX_BOUNCES_F32 + 1, 7, F32, p, p, p, None), abi.RT_ERR_UNSUPPORTED),
             ((ctx, 1 << 31, p, None, p, p, p, p, p, 0, 7, F32, p, p, p, None), abi.RT_ERR_UNSUPPORTED)]
    for args, want in cases:
        assert lib.rt_scatter_async(*args) == want and b"rt_scatter_async" in lib.rt_last_error()
        st = collect(renderer)
        assert st.kernel_id == 0 and st.samples == 0 and st.pixels == 0
    # n_rays == 0: RT_OK, nothing is enqueued (fp64 takes any bounce)
    assert lib.rt_scatter_async(ctx, 0, p, None, p, p, p, p, p, 1 << 20, 7, 0, p, p, p, None) == abi.RT_OK
    assert collect(renderer).kernel_id == 0
    out = renderer.scatter(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0), sc.table(), colour=np.zeros((0, 3)))
    assert out["origins"].shape == (0, 3) and out["colour"].shape == (0, 3)
    fresh = rt.GpuRenderer(lib=lib, precision="f32")   # no scene set
    try:
        assert lib.rt_scatter_async(fresh.ctx, 64, p, None, p, p, p, p, p, 0, 7, F32, p, p, p, None) == abi.RT_ERR_INVALID
        assert b"no scene" in lib.rt_last_error()
        assert lib.rt_path_step_async(fresh.ctx, 64, p, p, p, p, p, 0, 7, F32, p, p, p, p, p, None) == abi.RT_ERR_INVALID
        assert b"no scene" in lib.rt_last_error() and b"rt_path_step_async" in lib.rt_last_error()
    finally:
        fresh.close()
