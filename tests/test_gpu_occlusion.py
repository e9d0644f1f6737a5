"""Occlusion queries on the device (rt_query_occluded_async: occlusion_rays<T, ROOT2, MEGA>) against the oracle.
Bar: every byte equal; every comparison is np.testing.assert_array_equal on the uint8 arrays.

The expected byte is the header's equivalence (tests/occlusion_cases.py): 255 for a ray outside the query's
precondition or with a NaN t_max, else whether oracle_nearest_hit's closest t lies below t_max, strictly.
tests/test_occlusion_cases.py checks on the CPU that the launches below hold occluded and open rays in the same
batches, rays on every side of every bound, and whole batches that leave the sweep early.
Shapes are the smallest at which each part can go wrong: one ray, a partial batch, a full batch, a second batch with
one ray, five batches with a ragged end, and 600 000 rays (9 375 batches: more than 256 CUs hold waves at any
occupancy, so the stride loop takes a second trip; asserted from the occupancy the launch reports).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cull_cases as cc
import edge_scenes as es
import occlusion_cases as oc
import query_cases as qc
import rt_mi355x as rt
from rt_mi355x import abi

pytestmark = pytest.mark.gpu

F32 = abi.RT_FLAG_F32
WORK = ("box_groups", "filter_groups", "exact_tests", "cone_tests", "camera_exact_tests")


@pytest.fixture(autouse=True)
def _leave_the_shared_renderer_as_it_was(renderer):
    flags, seed = renderer.flags, renderer.seed
    yield
    renderer.flags, renderer.seed = flags, seed


def occluded(renderer, prec, o, d, flat, t_max=np.inf, root2=False):
    renderer.flags = F32 if prec == "f32" else 0
    out = renderer.occluded(o, d, flat, t_max=t_max, root2=root2)
    assert out.dtype == np.uint8 and out.shape == (np.asarray(d).shape[0],)
    return out


def same(got, want, what, la=None, tm=None):
    bad = np.flatnonzero(got != want)
    rows = ""
    if bad.size and la is not None:
        rows = "; ".join(f"ray {i} (batch {i // 64} lane {i % 64}): got {got[i]}, want {want[i]}, t_max {tm[i]!r}, "
                         f"o {la.o[i].tolist()} d {la.d[i].tolist()}" for i in bad[:6])
    np.testing.assert_array_equal(got, want, err_msg=f"{what}: {bad.size} rays differ; {rows}")


# ---------------------------------------------------------------- 1. adversarial rays
@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("fam", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.SCENES)
def test_adversarial(renderer, name, fam, kind, prec):
    """query_cases' launches (cull_cases' grazing rays, near-equal roots, degenerate lanes, silhouettes), both modes,
    t_max +inf everywhere and t_max by class; a camera family's shared origin gives the per-ray form's bytes."""
    for mode in qc.MODES:
        for how in oc.ASSIGNMENTS:
            la, tm, want = oc.case(name, fam, prec, kind, mode, how)
            got = occluded(renderer, prec, la.o, la.d, la.sc.flat, t_max=tm, root2=mode == "root2")
            same(got, want, f"{name}/{fam}/{kind}/{prec}/{mode}/{how}", la, tm)
            k = abi.kernel_info(renderer.query_stats.kernel_id)
            assert k["occlusion"] and k["mega"] is (la.sc.counts["n_mg"] > 0) and not k["camq"] and not k["query"]
            if la.centre is not None:
                shared = occluded(renderer, prec, la.centre, la.d, la.sc.flat, t_max=tm, root2=mode == "root2")
                same(shared, got, f"{name}/{fam}/{kind}/{prec}/{mode}/{how}: shared origin against per-ray origins", la, tm)
                assert not abi.kernel_info(renderer.query_stats.kernel_id)["camq"]   # the general sweep: no camera tables
                assert renderer.query_stats.cone_tests == 0 and renderer.query_stats.camera_exact_tests == 0


# ---------------------------------------------------------------- 2. one t_max for every ray
@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("name", ["b_supers", "d_mega"])
def test_scalar_t_max(renderer, name, prec):
    """d_t_max NULL: +inf, the launch's median hit t, and 0.0 (nothing is traced)."""
    la = qc.launch(name, "graze", prec, "mixed")
    for mode in qc.MODES:
        idx, t = la.ref[mode]
        median = float(np.median(t[idx >= 0]))
        for bound in (np.inf, median, 0.0):
            got = occluded(renderer, prec, la.o, la.d, la.sc.flat, t_max=bound, root2=mode == "root2")
            want = oc.expected(la.valid, t, np.full(la.n, bound, la.d.dtype))
            same(got, want, f"{name}/{prec}/{mode}/t_max {bound}")
            st = renderer.query_stats
            assert st.samples == int(la.valid.sum()) and (st.lane_slots == 0) is (bound == 0.0)
        assert 0.2 < (oc.expected(la.valid, t, np.full(la.n, median, la.d.dtype)) == oc.YES).mean() < 0.8


# ---------------------------------------------------------------- 3. shapes
SHAPES = [1, 63, 64, 65, 300, 600000]
N_CU = 256   # an MI355X
_shape_refs = {}


def shape_rays(prec):
    """600 000 plain rays into cull_cases' b_supers scene, their reference t (packed) and a t_max per ray around it,
    once; a smaller n takes a prefix."""
    if prec not in _shape_refs:
        sc, dtype = cc.scene("b_supers"), cc.DTYPES[prec]
        rays = cc.random_rays(sc, dtype, SHAPES[-1])
        o, d = np.ascontiguousarray(rays.o.T), np.ascontiguousarray(rays.d.T)
        idx, t = qc.oracle_nearest_hit(sc.flat, "packed", rays.o, rays.d)
        assert qc.valid_fast(o, d).all()
        tm = oc.assign(idx, t, "classes")
        want = oc.expected(np.ones(rays.n, bool), t, tm)
        for a in (o, d, tm, want):
            a.setflags(write=False)
        _shape_refs[prec] = (sc, o, d, tm, want)
    return _shape_refs[prec]


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("n", SHAPES)
def test_shapes(renderer, n, prec):
    sc, o, d, tm, want = shape_rays(prec)
    got = occluded(renderer, prec, o[:n], d[:n], sc.flat, t_max=tm[:n])
    same(got, want[:n], f"{n} rays")
    st = renderer.query_stats
    assert st.pixels == n and st.samples == int((want[:n] != oc.INVALID).sum()) == st.ray_segments
    go = oc.enters(np.ones(n, bool), tm[:n])
    assert st.lane_slots == 64 * sum(1 for b in range(0, n, 64) if go[b:b + 64].any())
    if n == SHAPES[-1]:   # more batches than the grid has waves: `batch += nw` takes a second trip
        assert (n + 63) // 64 > 4 * N_CU * st.kernel_wg_per_cu, st.kernel_wg_per_cu
        assert 0.1 < (want == oc.YES).mean() < 0.5 and (want == oc.INVALID).mean() > 0.05


def test_zero_rays(renderer):
    sc = cc.scene("b_supers")
    out = occluded(renderer, "f32", np.zeros((0, 3)), np.zeros((0, 3)), sc.flat)
    assert out.shape == (0,)
    lib, ctx, p = renderer.lib, renderer.ctx, ctypes.c_void_p(16)   # n_rays == 0: RT_OK, nothing is enqueued
    assert lib.rt_query_occluded_async(ctx, 0, p, None, p, None, 1.0, F32, p, None) == abi.RT_OK
    st = abi.RtStats()
    abi.check(lib, lib.rt_context_collect(ctx, None, ctypes.byref(st)))
    assert st.kernel_id == 0 and st.pixels == 0 and st.samples == 0


# ---------------------------------------------------------------- 4. plain scenes
EMPTY = lambda: rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32),   # noqa: E731
                             [rt.Lambertian((0.5, 0.5, 0.5))])


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("which", ["radii", "empty"])
def test_plain_scenes(renderer, which, prec):
    """The empty scene gives all 0; edge_scenes.radii (negative, zero and tiny radii) against the oracle, both origin
    forms, both modes, t_max +inf and by class."""
    flat, cam = (EMPTY(), es.camera(24, 10)) if which == "empty" else es.radii(24, 10)
    dtype = cc.DTYPES[prec]
    rng = np.random.default_rng(len(which))
    centre, d = qc.pixel_centre_rays(cam, [(c, r) for r in range(10) for c in range(24)], dtype)
    d = (d * 10.0 ** rng.uniform(-2, 2, (240, 1))).astype(dtype)
    o = (centre[None, :] + rng.uniform(-0.5, 0.5, (240, 3))).astype(dtype)
    for shared in (True, False):
        o_t = np.ascontiguousarray(np.broadcast_to(centre.astype(dtype), d.shape)) if shared else o
        assert qc.valid_rays(o_t, d).all()
        for mode in qc.MODES:
            idx, t = qc.oracle_nearest_hit(flat, mode, np.ascontiguousarray(o_t.T), np.ascontiguousarray(d.T))
            for how in oc.ASSIGNMENTS:
                tm = oc.assign(idx, t, how)
                got = occluded(renderer, prec, centre if shared else o, d, flat, t_max=tm, root2=mode == "root2")
                same(got, oc.expected(np.ones(240, bool), t, tm), f"{which}/{prec}/{mode}/{how}/shared {shared}")
                if which == "empty":
                    assert not got[~np.isnan(tm)].any()
                elif how == "inf":
                    assert any(flat.radius[i] < 0 for i in set(idx[idx >= 0].tolist())) and 0 < got.sum() < 240


# ---------------------------------------------------------------- 5. the early exit, from the counters
@pytest.mark.parametrize("name,prec", [("b_supers", "f32"), ("b_supers", "f64"), ("d_mega", "f32")])
def test_early_exit(renderer, name, prec):
    """128 valid rays with t_max +inf, each with an accepted root on the scene's one always-exact sphere: every lane is
    done after the always-exact group, so the wave leaves before its first box test, where the closest-hit query
    walks on."""
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    assert sc.counts["n_xs"] == 1 and sc.cluster_of()[0] == -1   # sphere 0, the ground, is the always-exact one
    o, d = oc.ground_rays(sc, dtype)
    assert o.shape == (128, 3) and qc.valid_rays(o, d).all()
    idx, t = qc.oracle_nearest_hit(sc.single(0), "packed", np.ascontiguousarray(o.T), np.ascontiguousarray(d.T))
    assert (idx == 0).all() and np.isfinite(t).all()   # an accepted root on that sphere alone, ray by ray
    got = occluded(renderer, prec, o, d, sc.flat)
    same(got, np.ones(128, np.uint8), f"{name}/{prec}")
    st = renderer.query_stats
    assert st.box_groups == 0 and st.filter_groups == 0, (st.box_groups, st.filter_groups)
    assert st.exact_tests > 0 and st.lane_slots == 128 and st.samples == 128
    renderer.query(o, d, sc.flat, want=("t",))
    assert renderer.query_stats.box_groups > 0


# ---------------------------------------------------------------- 6. stats
@pytest.mark.parametrize("prec", qc.PRECS)
def test_stats_of_an_untraced_launch(renderer, prec):
    """Every ray's t_max <= 0.001: no lane slots, no work, samples = the valid rays."""
    sc, dtype = cc.scene("b_supers"), cc.DTYPES[prec]
    rays = cc.random_rays(sc, dtype, 64 * 3 + 5)
    o, d = np.ascontiguousarray(rays.o.T), np.ascontiguousarray(rays.d.T).copy()
    d[7] = np.nan
    d[100] = 0
    n = d.shape[0]
    tm = np.array([0.001, np.nextafter(dtype(0.001), dtype(0)), 0.0, -0.0, -1.0, -np.inf, 1e-30], dtype)[np.arange(n) % 7]
    got = occluded(renderer, prec, o, d, sc.flat, t_max=tm)
    want = np.zeros(n, np.uint8)
    want[[7, 100]] = oc.INVALID
    same(got, want, "untraced")
    st = renderer.query_stats
    assert st.pixels == n and st.samples == n - 2 and st.ray_segments == n - 2 and st.lane_slots == 0 and st.bounce_iters == 0
    assert all(getattr(st, w) == 0 for w in WORK) and abi.RT_KERNEL_OCCLUSION(st.kernel_id)
    tm = tm.copy()
    tm[64 * 2 + 1] = np.nan   # a NaN bound: an invalid ray, not a sample
    tm[64 + 3] = 5.0          # one ray enters the sweep: its batch, and only its batch, holds lane slots
    got = occluded(renderer, prec, o, d, sc.flat, t_max=tm)
    st = renderer.query_stats
    assert got[64 * 2 + 1] == oc.INVALID and st.samples == n - 3 and st.lane_slots == 64 and st.exact_tests > 0


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("root2", [False, True])
def test_stats(renderer, prec, root2):
    dtype = cc.DTYPES[prec]
    for name, mega in (("b_supers", False), ("d_mega", True)):
        sc = cc.scene(name)
        rays = cc.random_rays(sc, dtype, 64 * 5 + 7)
        P = cc.camera_centre(sc, dtype, "outside_0")[0]
        o, d = np.ascontiguousarray(rays.o.T), np.ascontiguousarray(rays.d.T).copy()
        d[64:128] = np.nan          # a batch without a valid lane: not traced, no lane slots
        d[130] = 0                  # and two invalid lanes elsewhere
        d[64 * 5 + 3, 1] = np.inf
        n, n_valid = d.shape[0], d.shape[0] - 66
        for shared in (False, True):
            occluded(renderer, prec, P.astype(np.float64) if shared else o, d, sc.flat, root2=root2)
            st = renderer.query_stats
            k = abi.kernel_info(st.kernel_id)
            assert abi.RT_KERNEL_OCCLUSION(st.kernel_id) == 1 and k["occlusion"]
            assert k["T"] == ("float" if prec == "f32" else "double") and k["W"] == (5 if prec == "f32" else 4)
            assert k["root2"] is root2 and k["mega"] is mega and not k["camq"] and k["mode"] == 0
            assert not (k["split"] or k["items"] or k["guides"] or k["query"] or k["rays"])
            b = lambda x: "true" if x else "false"   # noqa: E731
            assert abi.kernel_name(st.kernel_id) == f"occlusion_rays<{k['T']},{b(root2)},{b(mega)}>"
            assert st.pixels == n and st.samples == n_valid and st.ray_segments == n_valid
            assert st.bounce_iters == 0 and st.direct_sky_samples == 0 and st.lane_slots == 64 * 5
            assert st.kernel_wg_per_cu >= k["W"] and st.kernel_ms > 0
            assert st.box_groups > 0 and st.exact_tests > 0 and st.cone_tests == 0 and st.camera_exact_tests == 0
    st = abi.RtStats()   # a collect after it starts from zero
    abi.check(renderer.lib, renderer.lib.rt_context_collect(renderer.ctx, None, ctypes.byref(st)))
    assert st.kernel_id == 0 and st.samples == 0 and st.pixels == 0 and st.ray_segments == 0


def test_refusals_on_a_live_context(renderer):
    lib, ctx = renderer.lib, renderer.ctx
    flat = rt.scenes.random_spheres(100).flatten()
    d = np.ascontiguousarray(cc.random_rays(cc.scene("a_one_super"), np.float32, 64).d.T)
    good = occluded(renderer, "f32", np.zeros(3), d, flat)
    p = ctypes.c_void_p(16)
    o3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nan = float("nan")
    cases = [((ctx, 64, None, o3, p, None, 1.0, abi.RT_FLAG_MODE_SCALAR | F32, p, None), abi.RT_ERR_UNSUPPORTED),
             ((ctx, 64, None, o3, p, None, 1.0, 0x40, p, None), abi.RT_ERR_INVALID),
             ((ctx, 64, p, o3, p, None, 1.0, F32, p, None), abi.RT_ERR_INVALID),
             ((ctx, 64, None, o3, p, None, nan, F32, p, None), abi.RT_ERR_INVALID),
             ((ctx, 64, None, o3, p, None, 1.0, F32, None, None), abi.RT_ERR_INVALID),
             ((ctx, 1 << 31, None, o3, p, None, 1.0, F32, p, None), abi.RT_ERR_UNSUPPORTED)]
    for args, want in cases:
        assert lib.rt_query_occluded_async(*args) == want
        assert b"rt_query_occluded_async" in lib.rt_last_error()
        st = abi.RtStats()
        abi.check(lib, lib.rt_context_collect(ctx, None, ctypes.byref(st)))
        assert st.kernel_id == 0 and st.samples == 0 and st.pixels == 0
    same(occluded(renderer, "f32", np.zeros(3), d, flat), good, "after the refusals")
    fresh = rt.GpuRenderer(lib=lib, precision="f32")   # no scene set
    try:
        assert lib.rt_query_occluded_async(fresh.ctx, 64, None, o3, p, None, 1.0, F32, p, None) == abi.RT_ERR_INVALID
        assert b"no scene" in lib.rt_last_error() and b"rt_query_occluded_async" in lib.rt_last_error()
    finally:
        fresh.close()


# ---------------------------------------------------------------- 7. device arrays
@pytest.mark.parametrize("prec", qc.PRECS)
def test_occluded_into_with_torch_tensors(prec):
    """Torch device tensors, in place, on a non-default torch stream, t_max as a number and as a tensor: the bytes of
    occluded() with numpy.  In a process of its own (tests/occluded_into_child.py)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "occluded_into_child.py")
    run = subprocess.run([sys.executable, child, prec], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "occluded_into ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


# ---------------------------------------------------------------- 8. inside a progressive session
@pytest.mark.parametrize("prec", qc.PRECS)
def test_inside_a_progressive_session(renderer, prec):
    """An occlusion query inside an open session leaves snapshot(), the counts and the session's next image
    unchanged, and gives the bytes it gives alone."""
    flat = rt.scenes.random_spheres(100).flatten()
    cam = es.camera(16, 9)
    centre, d = qc.pixel_centre_rays(cam, [(c, r) for r in range(9) for c in range(16)], cc.DTYPES[prec])
    renderer.seed, renderer.flags = es.SEED, F32 if prec == "f32" else 0
    want = renderer.render_flat(8, 16, flat, cam, want_linear=True)
    alone = occluded(renderer, prec, centre, d, flat, t_max=12.0)
    assert 0 < alone.sum() < alone.size
    renderer.flags = F32 if prec == "f32" else 0
    with renderer.begin_progressive(8, 16, flat, cam) as s:
        s.extend(8, image=False)
        before = s.snapshot(want_linear=True)
        counts = s.counts
        inside = occluded(renderer, prec, centre, d, flat, t_max=12.0)
        renderer.flags = F32 if prec == "f32" else 0
        after = s.snapshot(want_linear=True)
        qc.assert_same(after[0], before[0], "snapshot rgb")
        qc.assert_same(after[1], before[1], "snapshot linear")
        qc.assert_same(s.counts, counts, "counts")
        rgb, lin, _, rc = s.extend(16, want_linear=True)
    assert rc == want[3]
    qc.assert_same(rgb, want[0], "rgb")
    qc.assert_same(lin, want[1], "linear")
    same(inside, alone, "inside the session")
