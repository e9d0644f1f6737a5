"""rt_path_step_async on the device (path_step_rays<T, ROOT2, MEGA>).  Bar: 0 ulp; every comparison is
query_cases.assert_same (the values and the bit patterns).

  * fused equals the pair: every output array of the fused call equals rt_query_hits_async followed by rt_scatter_async
    on the same arrays.  On the mega-level scene of tests/test_gpu_query.py (cull_cases' d_mega: the MEGA kernels) with
    the adversarial launches of tests/query_cases.py, invalid lanes among them; on the 100-sphere scene (all three
    materials) with a camera's primary rays and the rays they scatter into, step after step, with invalid lanes put
    among them (the adversarial rays are aimed at cull_cases' own scenes);
  * the loop equals the render: integrators.path_trace over the camera's own primary rays against rt_render_async in
    mode "vectorized" and against the oracle (tests/test_step_cases.py proves that expectation on the CPU);
  * torch tensors on a torch stream, in a child process; direct_light with every shadow ray occluded.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import query_cases as qc
import step_cases as stc
from query_cases import assert_same
from rt_mi355x import abi, integrators

pytestmark = pytest.mark.gpu

F32 = abi.RT_FLAG_F32
OPTIONAL = ("index", "t", "normal", "front")
SEED = stc.SEED


@pytest.fixture(autouse=True)
def _leave_the_shared_renderer_as_it_was(renderer):
    flags, seed = renderer.flags, renderer.seed
    yield
    renderer.flags, renderer.seed = flags, seed


def setup(renderer, prec):
    renderer.flags = F32 if prec == "f32" else 0
    renderer.seed = SEED


def pair(renderer, flat, o, d, pix, smp, bounce, colour, root2):
    """rt_query_hits_async, then rt_scatter_async on its index and t: what the fused call must equal."""
    q = renderer.query(o, d, flat, root2=root2, want=("t", "index", "normal", "front"))
    valid = int(renderer.query_stats.samples)
    s = renderer.scatter(o, d, q["index"], q["t"], flat, pixel=pix, sample=smp, bounce=bounce, colour=colour, root2=root2)
    assert renderer.query_stats.samples == int((q["index"] >= 0).sum())
    status = np.where(q["index"] >= 0, abi.RT_STEP_SCATTERED,
                      np.where(q["index"] == abi.RT_QUERY_MISS, abi.RT_STEP_MISSED, abi.RT_STEP_INVALID)).astype(np.uint8)
    return dict(q, status=status, origins=s["origins"], directions=s["directions"], colour=s["colour"]), valid


def check_fused(renderer, prec, flat, o, d, pix, smp, bounce, colour, root2, mega, what):
    want, valid = pair(renderer, flat, o, d, pix, smp, bounce, colour, root2)
    got = renderer.path_step(o, d, flat, pixel=pix, sample=smp, bounce=bounce, colour=colour, root2=root2)
    st = renderer.query_stats
    n = d.shape[0]
    for key in ("status", "index", "t", "normal", "front", "origins", "directions", "colour"):
        if want[key] is None:
            assert got[key] is None
        else:
            assert_same(got[key], want[key], f"{what}: {key}")
    assert st.pixels == n and st.samples == valid and st.ray_segments == valid and st.bounce_iters == 0
    k = abi.kernel_info(st.kernel_id)
    assert abi.RT_KERNEL_STEP(st.kernel_id) == 1 and k["step"] and not k["query"] and not k["scatter"] and not k["camq"]
    assert k["root2"] is root2 and k["mega"] is mega and k["W"] == (5 if prec == "f32" else 4)
    b = lambda x: "true" if x else "false"   # noqa: E731
    assert abi.kernel_name(st.kernel_id) == f"path_step_rays<{k['T']},{b(root2)},{b(mega)}>"
    assert st.kernel_wg_per_cu >= k["W"]
    return got, want


# ---------------------------------------------------------------- 1. fused equals the pair
@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("kind", ["mixed", "solo"])
@pytest.mark.parametrize("fam", qc.FAMILIES)
def test_fused_equals_the_pair_on_the_mega_scene(renderer, fam, kind, prec):
    la = qc.launch("d_mega", fam, prec, kind)
    assert la.sc.counts["n_mg"] > 0 and not la.valid.all()
    setup(renderer, prec)
    rng = np.random.default_rng(la.n)
    pix = rng.integers(0, 1 << 32, la.n, dtype=np.uint64).astype(np.uint32)
    smp = rng.integers(0, 1 << 20, la.n).astype(np.uint32)
    colour = rng.uniform(0.05, 1.0, (la.n, 3)).astype(la.d.dtype)
    for root2 in (False, True):
        got, want = check_fused(renderer, prec, la.sc.flat, la.o, la.d, pix, smp, 3, colour, root2, True,
                                f"d_mega/{fam}/{kind}/{prec}/root2={root2}")
        idx, t = la.ref["root2" if root2 else "packed"]
        assert_same(got["index"], idx, "index against the oracle")
        assert_same(got["t"], t, "t against the oracle")
        inv = ~la.valid
        assert (got["status"][inv] == abi.RT_STEP_INVALID).all() and (got["status"][la.valid] != abi.RT_STEP_INVALID).all()
        for key, src in (("origins", la.o), ("directions", la.d), ("colour", colour)):   # NaN lanes among them: the bits
            keep = got["status"] != abi.RT_STEP_SCATTERED
            assert_same(got[key][keep], src[keep], f"{key} of rays that were not scattered")
        assert (got["status"] == abi.RT_STEP_SCATTERED).any()
        assert (got["status"] == abi.RT_STEP_MISSED).any() or (fam == "camera:inside" and root2)   # query_cases: all hit


def spoiled(o, d, every=11):
    """Invalid lanes among valid ones: a NaN, an infinity, a zero direction, one too long, an infinite origin."""
    o, d = o.copy(), d.copy()
    n = d.shape[0]
    for j, lane in enumerate(range(5, n, every)):
        kind = j % 5
        if kind == 0:
            d[lane, j % 3] = np.nan
        elif kind == 1:
            d[lane, (j + 1) % 3] = -np.inf
        elif kind == 2:
            d[lane] = 0
        elif kind == 3:
            d[lane] = d[lane] * d.dtype.type(2000.0)
        else:
            o[lane, j % 3] = np.inf
    return o, d


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("root2", [False, True])
def test_fused_equals_the_pair_on_the_100_sphere_scene(renderer, prec, root2):
    """The camera's primary rays at 4 spp, then the rays they scatter into, three steps deep; from the second step on
    invalid lanes are put among them (and stay: an invalid ray is handed back as it came)."""
    flat = stc.scene()
    setup(renderer, prec)
    o, d, pix, smp = stc.primary_rays(prec, 4)
    colour = np.ones((d.shape[0], 3), d.dtype)
    seen = set()
    for k in range(3):
        if k == 1:
            o, d = spoiled(o, d)
        got, want = check_fused(renderer, prec, flat, o, d, pix, smp, k, colour, root2, False, f"s100/{prec}/step {k}")
        hit = got["index"][got["index"] >= 0]
        seen |= {flat.materials[flat.material[i]].kind for i in np.unique(hit)}
        if k >= 1:
            assert (got["status"] == abi.RT_STEP_INVALID).sum() >= d.shape[0] // 11 - 1
        o, d, colour = got["origins"], got["directions"], got["colour"]
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("n", [1, 64, 65])
def test_sizes(renderer, n, prec):
    flat = stc.scene()
    setup(renderer, prec)
    o, d, pix, smp = stc.primary_rays(prec, 1)
    pick = np.arange(40, 40 + n)   # the middle of the frame: hits and misses
    o, d = spoiled(o[pick], d[pick], every=13) if n > 1 else (o[pick], d[pick])
    got, _ = check_fused(renderer, prec, flat, o, d, pix[pick], smp[pick], 0, None, False, False, f"n = {n}")
    assert got["status"].shape == (n,) and got["origins"].shape == (n, 3) and got["colour"] is None
    assert renderer.query_stats.lane_slots == 64 * ((n + 63) // 64)


@pytest.mark.parametrize("prec", stc.PRECS)
def test_all_combinations_of_the_optional_outputs(renderer, prec):
    """No value depends on which outputs were asked for: the 16 subsets of index, t, normal and front (status with every
    other one), against the call with all of them."""
    flat = stc.scene()
    setup(renderer, prec)
    o, d, pix, smp = stc.primary_rays(prec, 1)
    o, d = spoiled(o[:100], d[:100])
    pix, smp = pix[:100], smp[:100]
    colour = np.full((100, 3), 0.5, d.dtype)
    full = renderer.path_step(o, d, flat, pixel=pix, sample=smp, bounce=2, colour=colour)
    assert {0, 1, 255} == set(full["status"].tolist())
    for r in range(len(OPTIONAL) + 1):
        for j, subset in enumerate(itertools.combinations(OPTIONAL, r)):
            want = subset + (("status",) if (r + j) % 2 else ())
            got = renderer.path_step(o, d, flat, pixel=pix, sample=smp, bounce=2, colour=colour, want=want)
            assert set(got) == set(want) | {"origins", "directions", "colour"}
            for key in got:
                assert_same(got[key], full[key], f"{key} with {want}")


def test_out_of_range_sample(renderer):
    """A sample >= 2^20 on a ray that hits: not scattered (status 0, the query's outputs still reported),
    RT_ERR_INVALID at the collect, the other rays untouched by it."""
    flat = stc.scene()
    setup(renderer, "f32")
    o, d, pix, smp = (a[:128].copy() for a in stc.primary_rays("f32", 1))
    colour = np.ones((128, 3), np.float32)
    base = renderer.path_step(o, d, flat, pixel=pix, sample=smp, colour=colour)
    lane = int(np.flatnonzero(base["status"] == abi.RT_STEP_SCATTERED)[5])
    smp[lane] = 1 << 20
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        A = lambda a: integrators.DeviceArray(dev, a)   # noqa: E731
        d_o, d_d, d_c = A(o), A(d), A(colour)
        d_st, d_i = A(np.full(128, 9, np.uint8)), A(np.zeros(128, np.int32))
        renderer.path_step_into(d_o, d_d, A(pix), A(smp), colour=d_c, status=d_st, index=d_i)
        st = abi.RtStats()
        assert renderer.lib.rt_context_collect(renderer.ctx, None, ctypes.byref(st)) == abi.RT_ERR_INVALID
        assert b"rt_path_step_async" in renderer.lib.rt_last_error()
        status, index = d_st.get(), d_i.get()
        others = np.arange(128) != lane
        assert status[lane] == abi.RT_STEP_MISSED and index[lane] == base["index"][lane] >= 0
        assert_same(status[others], base["status"][others], "status")
        assert_same(index, base["index"], "index")
        for got, was, key in ((d_o.get(), o, "origins"), (d_d.get(), d, "directions"), (d_c.get(), colour, "colour")):
            assert_same(got[lane], was[lane], f"{key} of the refused lane")
            assert_same(got[others], base[key][others], key)
    again = renderer.path_step(o, d, flat, pixel=pix, sample=np.zeros(128, np.uint32), colour=colour)   # the flag was reset
    assert_same(again["directions"], base["directions"], "a clean call after it")


# ---------------------------------------------------------------- 2. the loop equals the render
def device_loop(renderer, prec, mode, spp, bounces):
    flat, cam = stc.scene(), stc.camera()
    root2 = mode == "root2"
    renderer.seed = SEED
    renderer.flags = (F32 if prec == "f32" else 0) | stc.render_flags(prec, mode)
    _, lin, st, rc = renderer.render_flat(bounces, spp, flat, cam, want_linear=True)
    assert rc == abi.RT_OK and abi.kernel_info(st.kernel_id)["mode"] == 1
    renderer.flags = F32 if prec == "f32" else 0
    o, d, pix, smp = stc.primary_rays(prec, spp)
    stats = {}
    radiance = integrators.path_trace(renderer, o, d, pix, smp, bounces, flat, seed=SEED, root2=root2, stats=stats)
    assert stats["invalid"] == 0, "a lane reported 255"
    got = integrators.reduce_samples(radiance, stc.W * stc.H, spp)
    assert_same(got, lin, f"the loop against rt_render_async (vectorized) {prec} {mode} spp {spp}")
    want, segs = stc.render(prec, mode, spp, bounces)
    assert_same(got, want, "the loop against the oracle")
    assert stats["ray_segments"] == st.ray_segments == segs and stats["samples"] == segs
    assert 1 <= stats["steps"] <= bounces and stats["kernel_ms"] > 0
    return radiance


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("mode", stc.MODES)
@pytest.mark.parametrize("spp", stc.SPPS)
def test_the_loop_equals_the_render(renderer, prec, mode, spp):
    radiance = device_loop(renderer, prec, mode, spp, stc.BOUNCES)
    assert_same(radiance, stc.loop(prec, mode, spp).radiance, "per-ray radiance against the CPU loop")


@pytest.mark.parametrize("prec", stc.PRECS)
def test_the_long_loop_equals_the_render(renderer, prec):
    bounces, spp = stc.LONG
    device_loop(renderer, prec, "packed", spp, bounces)


# ---------------------------------------------------------------- 3. torch tensors on a torch stream
@pytest.mark.parametrize("prec", stc.PRECS)
def test_path_step_into_with_torch_tensors(prec):
    """Torch device tensors, in place, on a non-default torch stream: the values of path_step() and scatter() with
    numpy.  In a process of its own (tests/path_step_child.py), as tests/query_into_child.py is: torch has to be
    imported before the library is loaded."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "path_step_child.py")
    run = subprocess.run([sys.executable, child, prec], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "path_step_into ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


# ---------------------------------------------------------------- 4. direct_light
@pytest.mark.parametrize("prec", stc.PRECS)
def test_direct_light_with_every_shadow_ray_occluded(renderer, prec):
    """The light inside the ground sphere: a hit on the ground has the light behind its surface, a hit anywhere else
    has the ground in the way, so nothing is lit and the result is the unlit loop's; a light in the open adds light."""
    flat = stc.scene()
    assert flat.radius[0] == 1000.0 and tuple(flat.center[0]) == (0.0, -1000.0, 0.0)
    setup(renderer, prec)
    o, d, pix, smp = stc.primary_rays(prec, 4)
    stats, lit_stats = {}, {}
    dark = integrators.direct_light(renderer, o, d, pix, smp, stc.BOUNCES, flat, light=stc.LIGHT_INSIDE, seed=SEED,
                                    stats=stats)
    assert_same(dark, stc.loop(prec, "packed", 4).radiance, "the unlit loop")
    assert stats["shadow_rays"] == stc.lit_lanes(prec, stc.LIGHT_INSIDE)[1] > 0 and stats["invalid"] == 0
    assert stats["ray_segments"] == stc.render(prec, "packed", 4)[1]
    lit = integrators.direct_light(renderer, o, d, pix, smp, stc.BOUNCES, flat, light=stc.LIGHT_OPEN,
                                   intensity=(300.0, 300.0, 300.0), seed=SEED, stats=lit_stats)
    assert (lit >= dark).all() and (lit > dark).any(1).mean() > 0.2
    assert lit_stats["shadow_rays"] == stats["shadow_rays"]
