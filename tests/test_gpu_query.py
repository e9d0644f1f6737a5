"""Ray queries on the device (rt_query_hits_async: query_rays<T, ROOT2, SHARED, MEGA>) against brute force and an
independent restatement.  Bar: 0 ulp everywhere; every comparison is query_cases.assert_same
(np.testing.assert_array_equal on the values and on the bit patterns, NaN and inf patterns and signed zeros included).

  * t and index: oracle_nearest_hit, brute force over every sphere in scene order with the reference's arithmetic
    (modes packed and root2), on the adversarial rays of tests/cull_cases.py as tests/query_cases.py composes them
    (tests/test_query_abi.py checks those launches on the CPU); camera families go through the shared-origin path
    and the general path.
  * normal, point and front: under Q1 the whole definition restated on tests/independent_v2.py's hit_scene, under
    root2 PackedHitRecords::finalize restated on its primitives from the oracle's (index, t).
Shapes are the smallest at which each part can go wrong: one ray, a partial batch, a full batch, a second batch with
one ray, five batches with a ragged end, 400 000 rays, and 600 000 rays (9 375 batches: more than 256 CUs hold waves
at any occupancy, 8 192 at the most, so the stride loop takes a second trip in every kernel; test_shapes asserts it
from the occupancy each launch reports).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cull_cases as cc
import edge_scenes as es
import query_cases as qc
import rt_mi355x as rt
from rt_mi355x import abi
from query_cases import assert_same

pytestmark = pytest.mark.gpu

F32 = abi.RT_FLAG_F32
ALL = ("t", "index", "normal", "point", "front")
CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-ray-tracing_amd", "bin", "rt-render")
N_FINALIZE = 192   # rays of an adversarial launch whose finalize is restated in pure Python (at most 4096 a case)


@pytest.fixture(autouse=True)
def _leave_the_shared_renderer_as_it_was(renderer):
    flags, seed = renderer.flags, renderer.seed
    yield
    renderer.flags, renderer.seed = flags, seed


def query(renderer, prec, o, d, flat, root2=False, want=ALL):
    renderer.flags = F32 if prec == "f32" else 0
    out = renderer.query(o, d, flat, root2=root2, want=want)
    assert list(out) == list(want)
    return out


def report(la, mode, got, what):
    """None, or the first lanes whose (index, t) differs from the oracle's."""
    want_i, want_t = la.ref[mode]
    bad = np.flatnonzero((got["index"] != want_i) | (qc.bits(got["t"]) != qc.bits(want_t)))
    if bad.size == 0:
        return None
    rows = [f"ray {i} (batch {i // 64} lane {i % 64}, {'valid' if la.valid[i] else 'invalid'}, target {la.target[i]}): "
            f"query ({got['index'][i]}, {got['t'][i]!r}), oracle ({want_i[i]}, {want_t[i]!r}); o {la.o[i].tolist()} "
            f"d {la.d[i].tolist()}" for i in bad[:6]]
    return f"{what} [{mode}]: {bad.size} of {la.n} rays differ; " + "; ".join(rows)


def check_finalize(la, mode, prec, got, pick):
    o, d = la.o[pick], la.d[pick]
    if mode == "packed":   # the whole definition, independently: index and t too
        idx, t, normal, point, front = qc.restate_packed(la.sc.flat, o, d, prec)
        assert_same(got["index"][pick], idx, "index (hit_scene)")
        assert_same(got["t"][pick], t, "t (hit_scene)")
    else:
        normal, point, front = qc.finalize(la.sc.flat, o, d, la.ref[mode][0][pick], la.ref[mode][1][pick])
    assert_same(got["normal"][pick], normal, f"normal [{mode}]")
    assert_same(got["point"][pick], point, f"point [{mode}]")
    assert_same(got["front"][pick], front, f"front [{mode}]")


# ---------------------------------------------------------------- 1. adversarial rays
@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("fam", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.SCENES)
def test_adversarial(renderer, name, fam, kind, prec):
    """cull_cases' rays: grazing within the reference's rounding, roots an ulp apart in different clusters, the
    filter's zero basis and origins 1e15 away, silhouettes from a centre outside every sphere and inside one; 64
    unrelated rays per batch, cases between degenerate and missing lanes, and one valid lane among 63 NaN lanes."""
    la = qc.launch(name, fam, prec, kind)
    flat = la.sc.flat
    v = np.flatnonzero(la.valid)
    pick = v[:: max(1, v.size // N_FINALIZE)][:N_FINALIZE]
    reports = []
    for mode in qc.MODES:
        got = query(renderer, prec, la.o, la.d, flat, root2=mode == "root2")
        reports.append(report(la, mode, got, f"{name}/{fam}/{kind}/{prec}/general"))
        st = renderer.query_stats
        assert abi.kernel_info(st.kernel_id)["mega"] is (la.sc.counts["n_mg"] > 0) and not abi.kernel_info(st.kernel_id)["camq"]
        inv = ~la.valid
        for key in ("normal", "point", "front"):   # an invalid ray and a miss: zeros
            assert not got[key][inv].any() and not got[key][got["index"] < 0].any(), key
        if la.centre is not None:   # the shared-origin path: the camera sweep over the centre's tables
            shared = query(renderer, prec, la.centre, la.d, flat, root2=mode == "root2")
            reports.append(report(la, mode, shared, f"{name}/{fam}/{kind}/{prec}/shared"))
            assert abi.kernel_info(renderer.query_stats.kernel_id)["camq"]
            for key in ALL:
                assert_same(shared[key], got[key], f"{key}: shared origin against the general path [{mode}]")
        if not any(reports):
            check_finalize(la, mode, prec, got, pick)
    reports = [r for r in reports if r]
    assert not reports, "\n".join(reports)


# ---------------------------------------------------------------- 2. finalize on plain scenes
def material_scene():
    """One Lambertian, one Metal and one hollow Dielectric sphere side by side over a Lambertian ground."""
    return rt.Scene.from_list([
        rt.Sphere((0.0, -1000.0, 0.0), 1000.0, rt.Lambertian((0.5, 0.5, 0.5))),
        rt.Sphere((-4.0, 1.0, 0.0), 1.0, rt.Lambertian((0.4, 0.2, 0.1))),
        rt.Sphere((0.0, 1.0, 0.0), 1.0, rt.Metal((0.7, 0.6, 0.5), 0.3)),
        rt.Sphere((4.0, 1.0, 0.0), 1.0, rt.Dielectric(1.5, True)),
    ]).flatten()


EMPTY = lambda: rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32),   # noqa: E731
                             [rt.Lambertian((0.5, 0.5, 0.5))])
_plain = {}


def plain_case(which, prec):
    """(flat, shared origin [3] float64, o [n, 3], d [n, 3]): the pixel-centre rays of a 24 x 10 frame, scaled to
    lengths in 0.01 .. 100, then the same directions from origins scattered about the centre."""
    if (which, prec) not in _plain:
        flat, cam = {"materials": lambda: (material_scene(), es.camera(24, 10)), "radii": lambda: es.radii(24, 10),
                     "empty": lambda: (EMPTY(), es.camera(24, 10))}[which]()
        dtype = cc.DTYPES[prec]
        rng = np.random.default_rng(len(which))
        centre, d = qc.pixel_centre_rays(cam, [(c, r) for r in range(10) for c in range(24)], dtype)
        d = (d * 10.0 ** rng.uniform(-2, 2, (240, 1))).astype(dtype)
        o = (centre[None, :] + rng.uniform(-0.5, 0.5, (240, 3))).astype(dtype)
        _plain[which, prec] = (flat, centre, o, d)
    return _plain[which, prec]


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("which", ["materials", "radii", "empty"])
def test_finalize(renderer, which, prec):
    """All three material kinds, negative, zero and tiny radii (tests/edge_scenes.py) and an empty scene, through
    both paths and both modes, every output against the restatement."""
    flat, centre, o, d = plain_case(which, prec)
    dtype = cc.DTYPES[prec]
    for shared in (True, False):
        oo = centre if shared else o
        o_t = np.broadcast_to(centre.astype(dtype), d.shape) if shared else o
        assert qc.valid_rays(o_t, d).all()
        for mode in qc.MODES:
            got = query(renderer, prec, oo, d, flat, root2=mode == "root2")
            idx, t = qc.oracle_nearest_hit(flat, mode, np.ascontiguousarray(o_t.T), np.ascontiguousarray(d.T))
            assert_same(got["index"], idx, "index")
            assert_same(got["t"], t, "t")
            if mode == "packed":
                want = qc.restate_packed(flat, o_t, d, prec)
                assert_same(got["index"], want[0], "index (hit_scene)")
                assert_same(got["t"], want[1], "t (hit_scene)")
                normal, point, front = want[2:]
            else:
                normal, point, front = qc.finalize(flat, o_t, d, idx, t)
            assert_same(got["normal"], normal, "normal")
            assert_same(got["point"], point, "point")
            assert_same(got["front"], front, "front")
            hit = set(idx[idx >= 0].tolist())
            if which == "materials":
                assert {1, 2, 3} <= hit and (idx < 0).any()
                assert {flat.materials[flat.material[i]].kind for i in hit} == {0, 1, 2}
            elif which == "radii":
                assert any(flat.radius[i] < 0 for i in hit) and len(hit) >= 4
            else:
                assert not hit and np.isinf(got["t"]).all() and (got["index"] == -1).all()
                assert not got["normal"].any() and not got["point"].any() and not got["front"].any()
                assert not np.signbit(got["normal"]).any() and not np.signbit(got["point"]).any()


# ---------------------------------------------------------------- 3. shapes
SHAPES = [1, 63, 64, 65, 257, 400000, 600000]
N_CU = 256   # an MI355X
_shape_refs = {}


def shape_rays(prec):
    """600 000 plain rays into cull_cases' b_supers scene and their references, once; a smaller n takes a prefix."""
    if prec not in _shape_refs:
        sc, dtype = cc.scene("b_supers"), cc.DTYPES[prec]
        rays = cc.random_rays(sc, dtype, SHAPES[-1])
        P = cc.camera_centre(sc, dtype, "outside_0")[0]
        o, d = np.ascontiguousarray(rays.o.T), np.ascontiguousarray(rays.d.T)
        ref = {}
        for mode in qc.MODES:
            ref["general", mode] = qc.oracle_nearest_hit(sc.flat, mode, rays.o, rays.d)
            ref["shared", mode] = qc.oracle_nearest_hit(sc.flat, mode, np.repeat(P[:, None], rays.n, 1), rays.d)
        assert qc.valid_fast(o, d).all()
        for a in (o, d) + tuple(x for r in ref.values() for x in r):
            a.setflags(write=False)
        _shape_refs[prec] = (sc, P, o, d, ref)
    return _shape_refs[prec]


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("n", SHAPES)
def test_shapes(renderer, n, prec):
    sc, P, o, d, ref = shape_rays(prec)
    for mode in qc.MODES:
        for path, origins in (("general", o[:n]), ("shared", P.astype(np.float64))):
            got = query(renderer, prec, origins, d[:n], sc.flat, root2=mode == "root2", want=("index", "t"))
            idx, t = ref[path, mode]
            assert got["index"].shape == (n,) and got["t"].shape == (n,)
            assert_same(got["index"], idx[:n], f"index {path} {mode}")
            assert_same(got["t"], t[:n], f"t {path} {mode}")
            st = renderer.query_stats
            assert st.pixels == n and st.samples == n and st.lane_slots == 64 * ((n + 63) // 64)
            if n == SHAPES[-1]:   # more batches than the grid has waves: `batch += nw` takes a second trip
                assert (n + 63) // 64 > 4 * N_CU * st.kernel_wg_per_cu, (path, mode, st.kernel_wg_per_cu)
    hit = ref["general", "packed"][0]
    assert 0.2 < (hit >= 0).mean() < 1.0


def test_zero_rays(renderer):
    sc = cc.scene("b_supers")
    out = query(renderer, "f32", np.zeros((0, 3)), np.zeros((0, 3)), sc.flat)
    assert out["t"].shape == (0,) and out["normal"].shape == (0, 3) and out["index"].dtype == np.int32
    lib, ctx, p = renderer.lib, renderer.ctx, ctypes.c_void_p(16)   # n_rays == 0: RT_OK, nothing is enqueued
    assert lib.rt_query_hits_async(ctx, 0, p, None, p, F32, p, p, p, p, p, None) == abi.RT_OK
    st = abi.RtStats()
    abi.check(lib, lib.rt_context_collect(ctx, None, ctypes.byref(st)))
    assert st.kernel_id == 0 and st.pixels == 0 and st.samples == 0


# ---------------------------------------------------------------- 4. invalid rays
def _square(x):
    return x.dtype.type(x * x)


def boundary_directions(dtype):
    """Directions (x, y, 0) whose |d|^2 in the type is exactly a bound, and the nearest ones just outside:
    {name: direction}.  1e6 = 1000^2 is exact; for 1e-6 (no exact square) x is the largest value whose square rounds
    below the bound and y^2 fills the gap in the fused add."""
    t = dtype
    T = qc.scalar_type(dtype)
    lo, hi = t(1e-6), t(1e6)
    out = {"at_max": np.array([1000, 0, 0], dtype), "above_max": np.array([np.nextafter(t(1000), t(np.inf)), 0, 0], dtype)}
    x = np.sqrt(lo)
    while _square(x) >= lo:
        x = np.nextafter(x, t(0))
    out["below_min"] = np.array([x, 0, 0], dtype)
    gap = float(lo) - float(x) * float(x)
    found = None
    for k in range(-64, 65):
        y = t(np.sqrt(gap))
        for _ in range(abs(k)):
            y = np.nextafter(y, t(np.inf) if k > 0 else t(0))
        if qc.iv.pk_len2((T(x), T(y), T(0))) == T(lo):
            found = y
            break
    assert found is not None
    out["at_min"] = np.array([x, found, 0], dtype)
    return out


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("shared", [False, True])
def test_invalid_rays(renderer, prec, shared):
    """One invalid lane of each kind in a batch of 64 gives -2 and NaN (zeros elsewhere); the bounds themselves are
    valid and traced; the other 63 results are those of the batch without it."""
    sc, P, o, d, ref = shape_rays(prec)
    dtype = cc.DTYPES[prec]
    n = 64 * 3   # the middle batch holds the lane; its neighbours must not notice either
    o0, d0 = o[:n].copy(), d[:n].copy()
    origins = P.astype(np.float64) if shared else o0
    base = query(renderer, prec, origins, d0, sc.flat, root2=True)
    b = boundary_directions(dtype)
    nan, inf = dtype(np.nan), dtype(np.inf)
    kinds = {"nan": (np.array([nan, 0, 1], dtype), False), "nan_z": (np.array([0.5, 0.5, nan], dtype), False),
             "inf": (np.array([1, -inf, 0], dtype), False), "zero": (np.zeros(3, dtype), False),
             "neg_zero": (np.array([-0.0, 0.0, -0.0], dtype), False),
             "below_min": (b["below_min"], False), "above_max": (b["above_max"], False),
             "at_min": (b["at_min"], True), "at_max": (b["at_max"], True)}
    for lane, (what, (dv, ok)) in zip((64, 95, 96, 127, 70, 100, 111, 64, 127), kinds.items()):
        dd = d0.copy()
        dd[lane] = dv
        o_t = np.broadcast_to(P, dd.shape) if shared else o0
        assert bool(qc.valid_rays(o_t[lane:lane + 1], dd[lane:lane + 1])[0]) is ok, what
        got = query(renderer, prec, origins, dd, sc.flat, root2=True)
        others = np.arange(n) != lane
        for key in ALL:
            assert_same(got[key][others], base[key][others], f"{what}: the other lanes' {key}")
        if ok:
            idx, t = qc.oracle_nearest_hit(sc.flat, "root2", np.ascontiguousarray(o_t[lane:lane + 1].T),
                                           np.ascontiguousarray(dd[lane:lane + 1].T))
            assert_same(got["index"][lane:lane + 1], idx, what)
            assert_same(got["t"][lane:lane + 1], t, what)
            assert renderer.query_stats.samples == n
        else:
            assert got["index"][lane] == abi.RT_QUERY_INVALID == -2 and np.isnan(got["t"][lane]), what
            assert not got["normal"][lane].any() and not got["point"][lane].any() and got["front"][lane] == 0, what
            assert renderer.query_stats.samples == n - 1 and renderer.query_stats.ray_segments == n - 1
    if not shared:   # origins: inf and NaN components
        for lane, val in ((64, inf), (127, -inf), (99, nan)):
            oo = o0.copy()
            oo[lane, lane % 3] = val
            got = query(renderer, prec, oo, d0, sc.flat, root2=True)
            others = np.arange(n) != lane
            for key in ALL:
                assert_same(got[key][others], base[key][others], f"origin {val}: the other lanes' {key}")
            assert got["index"][lane] == -2 and np.isnan(got["t"][lane]) and not got["point"][lane].any()
    else:            # a shared origin that is not finite: every ray is invalid, nothing is traced
        for bad in ((np.inf, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, 1e300 if prec == "f32" else -np.inf)):
            got = query(renderer, prec, np.array(bad), d0, sc.flat, root2=True)
            assert (got["index"] == -2).all() and np.isnan(got["t"]).all() and not got["normal"].any()
            st = renderer.query_stats
            assert st.samples == 0 and st.ray_segments == 0 and st.lane_slots == 0 and st.pixels == n
        again = query(renderer, prec, origins, d0, sc.flat, root2=True)   # the centre's tables are intact
        for key in ALL:
            assert_same(again[key], base[key], key)


# ---------------------------------------------------------------- 5. output independence
@pytest.mark.parametrize("prec", qc.PRECS)
def test_output_subsets(renderer, prec):
    """Outputs asked for alone equal outputs asked for together."""
    sc, P, o, d, _ = shape_rays(prec)
    n = 257
    for origins in (o[:n], P.astype(np.float64)):
        full = query(renderer, prec, origins, d[:n], sc.flat)
        assert (full["index"] >= 0).any() and (full["index"] < 0).any()
        for name in ALL:
            one = query(renderer, prec, origins, d[:n], sc.flat, want=(name,))
            assert_same(one[name], full[name], name)
        two = query(renderer, prec, origins, d[:n], sc.flat, want=("point", "index"))
        assert_same(two["point"], full["point"], "point")
        assert_same(two["index"], full["index"], "index")


# ---------------------------------------------------------------- 6. interleaving
@pytest.fixture(scope="module")
def scene_100():
    return rt.scenes.random_spheres(100).flatten()


@pytest.mark.parametrize("prec", qc.PRECS)
def test_render_query_render(renderer, scene_100, prec):
    """A render, a query with another shared origin, the same render: a bit-identical image (the camera tables are
    rebuilt under the key rule both times), and the query's values are those of the general path."""
    cam = es.camera(16, 9)
    other = np.array([-10.0, 3.0, 14.0])
    centre, d = qc.pixel_centre_rays(es.camera(16, 9, center=tuple(other)), [(c, r) for r in range(9) for c in range(16)],
                                     cc.DTYPES[prec])
    renderer.seed, renderer.flags = es.SEED, F32 if prec == "f32" else 0
    first = renderer.render_flat(8, 4, scene_100, cam, want_linear=True)
    got = query(renderer, prec, other, d, scene_100, root2=True)
    renderer.flags = F32 if prec == "f32" else 0
    again = renderer.render_flat(8, 4, scene_100, cam, want_linear=True)
    assert_same(first[0], again[0], "rgb")
    assert_same(first[1], again[1], "linear")
    general = query(renderer, prec, np.broadcast_to(other.astype(cc.DTYPES[prec]), d.shape), d, scene_100, root2=True)
    assert (got["index"] >= 0).any()
    for key in ALL:
        assert_same(got[key], general[key], key)
    # ... and a query from the render's own centre, between two renders, leaves them alike too
    query(renderer, prec, np.array(rt.MAIN_CAMERA["center"]), d, scene_100)
    renderer.flags = F32 if prec == "f32" else 0
    third = renderer.render_flat(8, 4, scene_100, cam, want_linear=True)
    assert_same(first[1], third[1], "linear after a query from the camera's centre")


@pytest.mark.parametrize("prec", qc.PRECS)
def test_inside_a_progressive_session(renderer, scene_100, prec):
    """A query inside an open session leaves snapshot() and the counts unchanged, and the session goes on to the
    image a plain render gives."""
    cam = es.camera(16, 9)
    centre, d = qc.pixel_centre_rays(cam, [(c, r) for r in range(9) for c in range(16)], cc.DTYPES[prec])
    renderer.seed, renderer.flags = es.SEED, F32 if prec == "f32" else 0
    want = renderer.render_flat(8, 16, scene_100, cam, want_linear=True)
    alone = query(renderer, prec, np.array([1.0, 2.0, 3.0]), d, scene_100)
    renderer.flags = F32 if prec == "f32" else 0
    with renderer.begin_progressive(8, 16, scene_100, cam) as s:
        s.extend(8, image=False)
        before = s.snapshot(want_linear=True)
        counts = s.counts
        inside = query(renderer, prec, np.array([1.0, 2.0, 3.0]), d, scene_100)
        general = query(renderer, prec, np.broadcast_to(np.array([1.0, 2.0, 3.0]), d.shape), d, scene_100)
        renderer.flags = F32 if prec == "f32" else 0
        after = s.snapshot(want_linear=True)
        assert_same(after[0], before[0], "snapshot rgb")
        assert_same(after[1], before[1], "snapshot linear")
        assert_same(s.counts, counts, "counts")
        rgb, lin, _, rc = s.extend(16, want_linear=True)
    assert rc == want[3]
    assert_same(rgb, want[0], "rgb")
    assert_same(lin, want[1], "linear")
    for key in ALL:
        assert_same(inside[key], alone[key], key)
        assert_same(general[key], alone[key], key)


# ---------------------------------------------------------------- 7. stats
@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("root2", [False, True])
def test_stats(renderer, prec, root2):
    """pixels = rays, samples = ray_segments = the valid rays, no bounce iterations, 64 lane slots per batch that
    traced, the kernel id's fields, and the reused sweeps' counters."""
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
        assert qc.valid_fast(o, d).sum() == n_valid
        for shared in (False, True):
            query(renderer, prec, P.astype(np.float64) if shared else o, d, sc.flat, root2=root2)
            st = renderer.query_stats
            k = abi.kernel_info(st.kernel_id)
            assert abi.RT_KERNEL_QUERY(st.kernel_id) == 1 and k["query"]
            assert k["T"] == ("float" if prec == "f32" else "double") and k["W"] == (5 if prec == "f32" else 4)
            assert k["root2"] is root2 and k["camq"] is shared and k["mega"] is mega
            assert k["mode"] == 0 and not k["split"] and not k["items"] and not k["guides"]
            b = lambda x: "true" if x else "false"   # noqa: E731
            assert abi.kernel_name(st.kernel_id) == f"query_rays<{k['T']},{b(root2)},{b(shared)},{b(mega)}>"
            assert st.pixels == n and st.samples == n_valid and st.ray_segments == n_valid
            assert st.bounce_iters == 0 and st.direct_sky_samples == 0
            assert st.lane_slots == 64 * 5   # six batches, one of them idle
            assert st.kernel_wg_per_cu >= k["W"] and st.kernel_ms > 0
            if shared:
                assert st.cone_tests > 0 and st.box_groups == 0 and st.filter_groups == 0 and st.exact_tests == 0
            else:
                assert st.box_groups > 0 and st.exact_tests > 0 and st.cone_tests == 0 and st.camera_exact_tests == 0
    # a collect after it starts from zero
    st = abi.RtStats()
    abi.check(renderer.lib, renderer.lib.rt_context_collect(renderer.ctx, None, ctypes.byref(st)))
    assert st.kernel_id == 0 and st.samples == 0 and st.pixels == 0 and st.ray_segments == 0


def test_refusals_on_a_live_context(renderer, scene_100):
    lib, ctx = renderer.lib, renderer.ctx
    d = np.ascontiguousarray(cc.random_rays(cc.scene("a_one_super"), np.float32, 64).d.T)
    good = query(renderer, "f32", np.zeros(3), d, scene_100)
    p = ctypes.c_void_p(16)
    o3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    cases = [((ctx, 64, None, o3, p, abi.RT_FLAG_MODE_SCALAR | F32, p, p, p, p, p, None), abi.RT_ERR_UNSUPPORTED),
             ((ctx, 64, None, o3, p, 0x40, p, p, p, p, p, None), abi.RT_ERR_INVALID),
             ((ctx, 64, p, o3, p, F32, p, p, p, p, p, None), abi.RT_ERR_INVALID),
             ((ctx, 64, None, o3, p, F32, None, None, None, None, None, None), abi.RT_ERR_INVALID),
             ((ctx, 1 << 31, None, o3, p, F32, p, p, p, p, p, None), abi.RT_ERR_UNSUPPORTED)]
    for args, want in cases:
        assert lib.rt_query_hits_async(*args) == want
        assert b"rt_query_hits_async" in lib.rt_last_error()
        st = abi.RtStats()
        abi.check(lib, lib.rt_context_collect(ctx, None, ctypes.byref(st)))
        assert st.kernel_id == 0 and st.samples == 0 and st.pixels == 0
    again = query(renderer, "f32", np.zeros(3), d, scene_100)
    for key in ALL:
        assert_same(again[key], good[key], key)
    fresh = rt.GpuRenderer(lib=lib, precision="f32")   # no scene set
    try:
        assert lib.rt_query_hits_async(fresh.ctx, 64, None, o3, p, F32, p, p, p, p, p, None) == abi.RT_ERR_INVALID
        assert b"no scene" in lib.rt_last_error()
        with pytest.raises(RuntimeError, match="scene"):
            fresh.query_into(np.zeros(3), FakeArray(d, 16), t=FakeArray(np.zeros(64, np.float32), 16))
    finally:
        fresh.close()


class FakeArray:
    def __init__(self, a, ptr):
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": a.dtype.str, "data": (ptr, False), "version": 3}


# ---------------------------------------------------------------- 8. query_into
@pytest.mark.parametrize("prec", qc.PRECS)
def test_query_into_with_torch_tensors(prec):
    """Torch device tensors, in place, on a non-default torch stream: the values of query() with numpy.  In a process
    of its own (tests/query_into_child.py): torch brings a HIP runtime of its own and has to be imported before
    the library is loaded, and this session loaded the library long ago."""
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "query_into_child.py")
    run = subprocess.run([sys.executable, child, prec], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "query_into ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


# ---------------------------------------------------------------- 9. rt-render --pick
PICK = re.compile(r"^Pick \((\d+), (\d+)\): (?:(miss)|sphere (\d+) (\w+) t (\S+) point \[(\S+), (\S+), (\S+)\] "
                  r"normal \[(\S+), (\S+), (\S+)\] front ([01]))$")


@pytest.mark.parametrize("prec", qc.PRECS)
def test_cli_pick(tmp_path, lib, prec):
    """rt-render --pick prints, per pixel, what query() gives for the ray through the pixel's centre (shared origin,
    root2), and writes no image."""
    flat = material_scene()
    scene = rt.Scene.from_list([rt.Sphere(tuple(flat.center[i]), flat.radius[i], flat.materials[flat.material[i]])
                                for i in range(flat.n_spheres)])
    (tmp_path / "scene.toml").write_text(rt.scenes.scene_to_toml(scene))
    pixels = [(0, 0), (9, 4), (12, 4), (14, 3), (23, 9), (11, 9), (12, 4), (14, 4), (23, 4)]
    args = [CLI, "--scene", "scene.toml", "--width", "24", "--height", "10"] + (["--f32"] if prec == "f32" else [])
    for c, r in pixels:
        args += ["--pick", f"{c},{r}"]
    run = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert not list(tmp_path.glob("output*")) and not list(tmp_path.glob("*.png"))
    lines = [PICK.match(ln) for ln in run.stdout.splitlines() if ln.startswith("Pick ")]
    assert len(lines) == len(pixels) and all(lines), run.stdout
    dtype = cc.DTYPES[prec]
    cam = rt.camera_new_py(24, 10, **rt.MAIN_CAMERA)
    centre, d = qc.pixel_centre_rays(cam, pixels, dtype)
    g = rt.GpuRenderer(lib=lib, precision=prec)
    try:
        want = g.query(centre, d, flat, root2=True)
    finally:
        g.close()
    kinds = {0: "lambertian", 1: "metal", 2: "dielectric"}
    assert (want["index"] >= 0).sum() >= 4 and (want["index"] == -1).any()
    assert {1, 2, 3} <= set(want["index"].tolist())
    for k, m in enumerate(lines):
        assert (int(m.group(1)), int(m.group(2))) == pixels[k]
        if want["index"][k] < 0:
            assert m.group(3) == "miss"
            continue
        assert int(m.group(4)) == want["index"][k] and m.group(5) == kinds[flat.materials[flat.material[want["index"][k]]].kind]
        got = np.array([float(x) for x in m.group(6, 7, 8, 9, 10, 11, 12)]).astype(dtype)
        assert_same(got, np.concatenate([[want["t"][k]], want["point"][k], want["normal"][k]]).astype(dtype), f"pick {pixels[k]}")
        assert int(m.group(13)) == want["front"][k]
    for extra in (["--mode", "scalar"], ["--guides"], ["--pick", "24,0"], ["--pick", "3"], ["--out", "o.ppm"],
                  ["--block-size", "8"], ["--sample-parallel"], ["--progressive", "2"], ["--adaptive", "0.1", "--spp-min", "2"]):
        bad = subprocess.run(args + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and "--pick" in bad.stderr, (extra, bad.stderr)
