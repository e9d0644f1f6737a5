"""Ray lists on the device: rt_path_step_list_async (path_step_list<T, ROOT2, MEGA> and the compaction behind it) and
rt_ray_list_compact_async (keep_ballots, list_tile_sums, list_scan_tiles, list_scatter).  Bar: 0 ulp and byte-equal
lists; every comparison of reals is query_cases.assert_same (the values and the bit patterns).

  * expected ray values: rt_path_step_async (GpuRenderer.path_step) on a copy of the same inputs, which
    tests/test_gpu_path_step.py holds to the oracle; a listed ray equals it, an unlisted ray keeps every byte it had
    (inputs and the outputs' sentinels);
  * expected lists: numpy, list_in[:count][status[list_in[:count]] == 1] (stable in list position);
  * the scan's levels: through rt_ray_list_compact_async, whose keep mask sets the pattern exactly, at RT_LIST_TILE 64
    and 256 with sizes around a batch, a tile and list_scan_tiles' chunk (abi.LIST_SCAN_CHUNK tiles);
  * the loop: integrators.path_trace(compact=True) against compact=False and against a render in mode "vectorized".
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
from rt_mi355x.step_checks import STEP_NAMES, STEP_OUTPUTS, _step_shape
from test_gpu_path_step import spoiled

pytestmark = pytest.mark.gpu

F32 = abi.RT_FLAG_F32
SEED = stc.SEED
SENT = dict(status=9, index=7, t=7.0, normal=7.0, front=7)   # what the outputs hold before a call
WORD = 0xDEADBEEF                                             # ... and the output list and its count
RAYS = ("origins", "directions", "colour")
N = 300


@pytest.fixture(autouse=True)
def _leave_the_shared_renderer_as_it_was(renderer):
    flags, seed, tile = renderer.flags, renderer.seed, os.environ.pop("RT_LIST_TILE", None)
    yield
    renderer.flags, renderer.seed = flags, seed
    os.environ.pop("RT_LIST_TILE", None)
    if tile is not None:
        os.environ["RT_LIST_TILE"] = tile


def setup(renderer, prec):
    renderer.flags = F32 if prec == "f32" else 0
    renderer.seed = SEED


def rays(prec, n, first=200):
    """n rays of the 16 x 9 frame at 4 spp from row 3 on (misses, then hits), invalid lanes among them, a colour each."""
    o, d, pix, smp = stc.primary_rays(prec, 4)
    pick = np.arange(first, first + n)
    o, d = spoiled(o[pick], d[pick], every=13) if n > 1 else (o[pick].copy(), d[pick].copy())
    colour = np.random.default_rng(n).uniform(0.05, 1.0, (n, 3)).astype(d.dtype)
    return o, d, colour, pix[pick].copy(), smp[pick].copy()


def collect(renderer, expect=abi.RT_OK):
    st = abi.RtStats()
    assert renderer.lib.rt_context_collect(renderer.ctx, None, ctypes.byref(st)) == expect, renderer.lib.rt_last_error()
    return st


def list_step(renderer, arrs, bounce, lst=None, count=None, out=True, names=STEP_NAMES, root2=False, rc=abi.RT_OK):
    """One rt_path_step_list_async over copies of arrs = (o, d, colour, pixel, sample) with every output pre-filled.
    Returns ({name: array after the call}, RtStats)."""
    o, d, colour, pix, smp = arrs
    n = d.shape[0]
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        A = lambda a: integrators.DeviceArray(dev, a)   # noqa: E731
        dv = dict(origins=A(o), directions=A(d), colour=A(colour))
        outs = {k: A(np.full(_step_shape(k, n), SENT[k], STEP_OUTPUTS[k][1] or d.dtype)) for k in names}
        d_li = None if lst is None else A(np.ascontiguousarray(lst, dtype=np.uint32))
        d_ci = None if count is None else A(np.array([count], np.uint32))
        d_lo = A(np.full(n, WORD, np.uint32)) if out else None
        d_co = A(np.array([WORD], np.uint32)) if out else None
        assert renderer.path_step_list_into(dv["origins"], dv["directions"], A(pix), A(smp), bounce=bounce, list_in=d_li,
                                            count_in=d_ci, list_out=d_lo, count_out=d_co, colour=dv["colour"], root2=root2,
                                            **outs) == n
        st = collect(renderer, rc)
        got = {k: a.get() for k, a in itertools.chain(dv.items(), outs.items())}
        if out:
            got["list_out"], got["count_out"] = d_lo.get(), int(d_co.get()[0])
        if lst is not None:
            assert_same(d_li.get(), np.ascontiguousarray(lst, dtype=np.uint32), "the input list is only read")
    return got, st


def expectation(renderer, flat, arrs, bounce, lst=None, count=None, names=STEP_NAMES, root2=False):
    """What list_step must leave: rt_path_step_async's values at the listed rays, the bytes from before elsewhere."""
    o, d, colour, pix, smp = arrs
    n = d.shape[0]
    full = renderer.path_step(o, d, flat, pixel=pix, sample=smp, bounce=bounce, colour=colour, root2=root2)
    entries = (np.arange(n, dtype=np.uint32) if lst is None else np.asarray(lst, dtype=np.uint32))[:n if count is None else min(count, n)]
    listed = entries[entries < n]
    mask = np.zeros(n, bool)
    mask[listed] = True
    want = {}
    for key, src in zip(RAYS, (o, d, colour)):
        want[key] = src.copy()
        want[key][mask] = full[key][mask]
    for k in names:
        want[k] = np.full(_step_shape(k, n), SENT[k], STEP_OUTPUTS[k][1] or d.dtype)
        want[k][mask] = full[k][mask]
    want["list_out"] = listed[full["status"][listed] == abi.RT_STEP_SCATTERED]
    want["valid"] = int((full["status"][listed] != abi.RT_STEP_INVALID).sum())
    return want


def check_step(renderer, prec, flat, arrs, bounce, what, lst=None, count=None, out=True, names=STEP_NAMES, root2=False,
               rc=abi.RT_OK):
    want = expectation(renderer, flat, arrs, bounce, lst, count, names, root2)
    got, st = list_step(renderer, arrs, bounce, lst, count, out, names, root2, rc)
    n = arrs[1].shape[0]
    for key in RAYS + tuple(names):
        assert_same(got[key], want[key], f"{what}: {key}")
    if out:
        k = want["list_out"].size
        assert got["count_out"] == k, what
        assert_same(got["list_out"][:k], want["list_out"], f"{what}: list_out")
        assert (got["list_out"][k:] == WORD).all(), f"{what}: list_out past count_out was written"
    assert st.pixels == n and st.samples == want["valid"] and st.ray_segments == want["valid"] and st.bounce_iters == 0
    info = abi.kernel_info(st.kernel_id)
    assert abi.RT_KERNEL_LIST(st.kernel_id) == 1 and info["list"] and info["step"] and not info["query"] and not info["camq"]
    assert info["root2"] is root2 and info["W"] == (5 if prec == "f32" else 4) and st.kernel_wg_per_cu >= info["W"]
    b = lambda x: "true" if x else "false"   # noqa: E731
    assert abi.kernel_name(st.kernel_id) == f"path_step_list<{info['T']},{b(root2)},{b(info['mega'])}>"
    return got, want


# ---------------------------------------------------------------- 1. the identity list
@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_identity_list(renderer, n, prec):
    flat = stc.scene()
    setup(renderer, prec)
    arrs = rays(prec, n)
    got, want = check_step(renderer, prec, flat, arrs, 0, f"identity n = {n}")
    if n >= 63:
        assert 0 < want["list_out"].size < n
    again, _ = list_step(renderer, arrs, 0)
    for key in got:
        assert np.array_equal(np.asarray(got[key]).view(np.uint8) if isinstance(got[key], np.ndarray) else got[key],
                              np.asarray(again[key]).view(np.uint8) if isinstance(again[key], np.ndarray) else again[key]), key


# ---------------------------------------------------------------- 2. explicit lists
def explicit_lists():
    every_other = np.arange(0, N, 2)
    straddle = np.arange(40, 105)            # 65 rays over a batch boundary of the ray ids (and two batches of the list)
    short = np.full(N, 0xFFFFFFFF, np.uint32)
    short[:37] = np.random.default_rng(3).permutation(N)[:37]
    return [("empty", np.full(N, 0xFFFFFFFF, np.uint32), 0), ("one ray", np.full(N, 141, np.uint32), 1),
            ("every other ray", np.concatenate([every_other, np.full(N - every_other.size, WORD)]), every_other.size),
            ("65 rays straddling a batch", np.concatenate([straddle, np.zeros(N - 65)]), 65),
            ("decreasing", np.arange(N)[::-1], N), ("count_in shorter than the array", short, 37)]


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("case", range(6))
def test_explicit_lists(renderer, case, prec):
    what, lst, count = explicit_lists()[case]
    flat = stc.scene()
    setup(renderer, prec)
    got, want = check_step(renderer, prec, flat, rays(prec, N), 1, what, lst=lst, count=count)
    if count == 0:
        assert got["count_out"] == 0 and (got["status"] == SENT["status"]).all()
    elif count > 1:
        assert 0 < want["list_out"].size < count
        pos = {int(r): i for i, r in enumerate(np.asarray(lst, dtype=np.uint32)[:count])}
        order = [pos[int(r)] for r in got["list_out"][:got["count_out"]]]
        assert order == sorted(order), "list_out is stable with respect to list position"


@pytest.mark.parametrize("prec", stc.PRECS)
def test_no_output_list(renderer, prec):
    flat = stc.scene()
    setup(renderer, prec)
    arrs = rays(prec, N)
    check_step(renderer, prec, flat, arrs, 1, "no output list, identity", out=False)
    third = np.concatenate([np.arange(0, N, 3), np.full(N - 100, WORD)])   # a list has one word per ray: 100 listed, a tail
    check_step(renderer, prec, flat, arrs, 1, "no output list, every third ray", lst=third, count=100, out=False)


@pytest.mark.parametrize("prec", stc.PRECS)
def test_all_combinations_of_the_optional_outputs(renderer, prec):
    """The 16 subsets of index, t, normal and front (status with every other one) leave the same values."""
    flat = stc.scene()
    setup(renderer, prec)
    arrs = rays(prec, 100)
    lst = np.concatenate([np.arange(1, 100, 2), np.full(50, WORD)])
    full = expectation(renderer, flat, arrs, 2, lst, 50)
    assert {0, 1, 255} <= set(full["status"].tolist())
    optional = ("index", "t", "normal", "front")
    for r in range(len(optional) + 1):
        for j, subset in enumerate(itertools.combinations(optional, r)):
            names = subset + (("status",) if (r + j) % 2 else ())
            got, _ = list_step(renderer, arrs, 2, lst, 50, names=names)
            assert set(got) == set(names) | set(RAYS) | {"list_out", "count_out"}
            for key in names + RAYS:
                assert_same(got[key], full[key], f"{key} with {names}")
            assert_same(got["list_out"][:got["count_out"]], full["list_out"], f"list_out with {names}")


# ---------------------------------------------------------------- 3. bounds: ordinary inputs, not faults
@pytest.mark.parametrize("prec", stc.PRECS)
def test_an_entry_outside_the_arrays_is_skipped(renderer, prec):
    flat = stc.scene()
    setup(renderer, prec)
    arrs = rays(prec, N)
    for bad in (N, 0xFFFFFFFF):
        lst = np.arange(N, dtype=np.uint32)
        lst[150] = bad   # ray 150 is then not listed
        got, _ = check_step(renderer, prec, flat, arrs, 1, f"entry {bad:#x}", lst=lst, count=N, rc=abi.RT_ERR_INVALID)
        assert b"ray list" in renderer.lib.rt_last_error()
        assert bad not in got["list_out"][:got["count_out"]].tolist() and got["status"][150] == SENT["status"]
    check_step(renderer, prec, flat, arrs, 1, "a clean call after it: the flag was reset")


@pytest.mark.parametrize("prec", stc.PRECS)
def test_a_count_above_the_capacity_is_clamped(renderer, prec):
    flat = stc.scene()
    setup(renderer, prec)
    arrs = rays(prec, N)
    check_step(renderer, prec, flat, arrs, 1, "identity, count n + 7", count=N + 7, rc=abi.RT_ERR_INVALID)
    check_step(renderer, prec, flat, arrs, 1, "decreasing, count n + 7", lst=np.arange(N)[::-1], count=N + 7,
               rc=abi.RT_ERR_INVALID)
    check_step(renderer, prec, flat, arrs, 1, "decreasing, count 2^32 - 1", lst=np.arange(N)[::-1], count=0xFFFFFFFF,
               rc=abi.RT_ERR_INVALID)


# ---------------------------------------------------------------- 4. the scan's levels, through the compaction call
def keep_patterns(n):
    rng = np.random.default_rng(n)
    last_lane = np.zeros(n, np.uint8)
    last_lane[63::64] = 1
    only_last = np.zeros(n, np.uint8)
    only_last[n - 1] = 200   # any non-zero byte keeps
    return [("all", np.ones(n, np.uint8)), ("none", np.zeros(n, np.uint8)),
            ("alternating", (np.arange(n) % 2).astype(np.uint8)), ("the last lane of every batch", last_lane),
            ("only ray n - 1", only_last), ("random 0.5", (rng.random(n) < 0.5).astype(np.uint8)),
            ("random 0.01", (rng.random(n) < 0.01).astype(np.uint8) * 255)]


def check_compaction(renderer, n, form, patterns, what):
    lst = count = None
    if form == "permuted":
        count = n - n // 5 - 1   # < n
        lst = np.full(n, 0xFFFFFFFF, np.uint32)
        lst[:count] = np.random.default_rng(n + 1).permutation(n)[:count]
    entries = np.arange(n, dtype=np.uint32) if lst is None else lst[:count]
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        A = lambda a: integrators.DeviceArray(dev, a)   # noqa: E731
        d_li = None if lst is None else A(lst)
        d_ci = None if count is None else A(np.array([count], np.uint32))
        d_keep, d_lo, d_co = A(np.zeros(n, np.uint8)), A(np.zeros(n, np.uint32)), A(np.zeros(1, np.uint32))
        for name, keep in patterns:
            d_keep.set(keep)
            d_lo.set(np.full(n, WORD, np.uint32))
            d_co.set(np.array([WORD], np.uint32))
            assert renderer.compact_list_into(d_keep, d_lo, d_co, list_in=d_li, count_in=d_ci) == n
            st = collect(renderer)
            want = entries[keep[entries] != 0]
            got, k = d_lo.get(), int(d_co.get()[0])
            assert k == want.size, f"{what} {name}: count_out {k}, expected {want.size}"
            assert np.array_equal(got[:k], want), f"{what} {name}: list_out"
            assert (got[k:] == WORD).all(), f"{what} {name}: list_out past count_out was written"
            assert st.pixels == n and st.samples == 0 and st.ray_segments == 0 and st.lane_slots == 0
            assert st.kernel_id == 0x8000 | 1 << 18 and abi.kernel_info(st.kernel_id)["list"] and st.kernel_wg_per_cu == 0


@pytest.mark.parametrize("form", ["identity", "permuted"])
@pytest.mark.parametrize("tile", [64, 256])
def test_scan_levels(renderer, tile, form):
    """Sizes around a batch, a tile, and kernel 2's chunk of abi.LIST_SCAN_CHUNK tiles (the last size has one tile more
    than a chunk, so the running total is carried into a second chunk)."""
    os.environ["RT_LIST_TILE"] = str(tile)
    sizes = sorted({63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 65, (abi.LIST_SCAN_CHUNK + 1) * tile + 1})
    assert sizes[-1] > abi.LIST_SCAN_CHUNK * tile
    for n in sizes:
        check_compaction(renderer, n, form, keep_patterns(n), f"tile {tile} n {n} {form}")


def test_the_default_tile(renderer):
    assert "RT_LIST_TILE" not in os.environ
    n = 2 * abi.LIST_TILE_DEFAULT + 65
    pats = [p for p in keep_patterns(n) if p[0] in ("random 0.5", "only ray n - 1")]
    check_compaction(renderer, n, "identity", pats, "default tile")
    check_compaction(renderer, n, "permuted", pats[:1], "default tile")
    os.environ["RT_LIST_TILE"] = "100"   # not a power of two: ignored
    check_compaction(renderer, 1000, "permuted", keep_patterns(1000)[5:6], "an ignored RT_LIST_TILE")


def test_a_list_from_a_status_array(renderer):
    """d_list_in NULL, d_keep = d_status: the rays of a plain step that are not missed."""
    flat = stc.scene()
    setup(renderer, "f32")
    o, d, colour, pix, smp = rays("f32", N)
    status = renderer.path_step(o, d, flat, pixel=pix, sample=smp, want=("status",))["status"]
    check_compaction(renderer, N, "identity", [("status", status)], "keep = status")


# ---------------------------------------------------------------- 5. stale scratch
@pytest.mark.parametrize("prec", stc.PRECS)
def test_a_short_list_after_a_long_one(renderer, prec):
    """The ballot scratch still holds the words of the 300-ray step when the 5-ray step runs on the same context."""
    flat = stc.scene()
    setup(renderer, prec)
    arrs = rays(prec, N)
    first, want = check_step(renderer, prec, flat, arrs, 0, "the full list")
    assert want["list_out"].size > 64
    after = (first["origins"], first["directions"], first["colour"], arrs[3], arrs[4])
    five = first["list_out"][[0, 9, 17, 40, 70]]
    lst = np.concatenate([five, np.full(N - 5, WORD)])
    got, want = check_step(renderer, prec, flat, after, 1, "five rays", lst=lst, count=5)
    assert got["count_out"] == want["list_out"].size <= 5 and set(got["list_out"][:got["count_out"]].tolist()) <= set(five.tolist())


# ---------------------------------------------------------------- 6. the loop
def loops(renderer, prec, mode, spp, bounces):
    flat, cam = stc.scene(), stc.camera()
    root2 = mode == "root2"
    renderer.seed = SEED
    renderer.flags = (F32 if prec == "f32" else 0) | stc.render_flags(prec, mode)
    _, lin, st, rc = renderer.render_flat(bounces, spp, flat, cam, want_linear=True)
    assert rc == abi.RT_OK and abi.kernel_info(st.kernel_id)["mode"] == 1
    renderer.flags = F32 if prec == "f32" else 0
    o, d, pix, smp = stc.primary_rays(prec, spp)
    plain, listed = {}, {}
    want = integrators.path_trace(renderer, o, d, pix, smp, bounces, flat, seed=SEED, root2=root2, stats=plain)
    got = integrators.path_trace(renderer, o, d, pix, smp, bounces, flat, seed=SEED, root2=root2, stats=listed, compact=True)
    assert_same(got, want, f"compact=True against compact=False {prec} {mode} spp {spp}")
    for key in ("ray_segments", "samples", "steps", "invalid", "shadow_rays"):
        assert listed[key] == plain[key], (key, listed[key], plain[key])
    assert listed["invalid"] == 0 and listed["kernel_ms"] > 0 and 1 <= listed["steps"] <= bounces
    assert listed["ray_segments"] == st.ray_segments
    assert_same(integrators.reduce_samples(got, stc.W * stc.H, spp), lin, "the compacted loop against rt_render_async (vectorized)")


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("mode", stc.MODES)
@pytest.mark.parametrize("spp", stc.SPPS)
def test_the_compacted_loop_equals_the_loop_and_the_render(renderer, prec, mode, spp):
    loops(renderer, prec, mode, spp, stc.BOUNCES)


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("mode", stc.MODES)
def test_the_long_compacted_loop(renderer, prec, mode):
    bounces, spp = stc.LONG
    loops(renderer, prec, mode, spp, bounces)


def test_no_scene_is_refused(lib):
    import rt_mi355x as rt
    fresh = rt.GpuRenderer(lib=lib)
    try:
        p = ctypes.c_void_p(16)
        assert lib.rt_path_step_list_async(fresh.ctx, 64, None, None, p, p, p, p, p, 0, 7, F32, p, p, p, p, p, None, None,
                                           None) == abi.RT_ERR_INVALID
        assert b"rt_path_step_list_async" in lib.rt_last_error() and b"no scene" in lib.rt_last_error()
        assert lib.rt_path_step_list_async(fresh.ctx, 0, None, None, p, p, p, p, p, 0, 7, F32, p, p, p, p, p, None, None,
                                           None) == abi.RT_ERR_INVALID   # the no-scene check comes before n_rays == 0
    finally:
        fresh.close()


# ---------------------------------------------------------------- 7. torch tensors on a torch stream
@pytest.mark.parametrize("prec", stc.PRECS)
def test_path_step_list_into_with_torch_tensors(prec):
    """Torch device tensors on a non-default torch stream, two steps chained through the device count with no host read
    between them.  In a process of its own (tests/path_step_list_child.py), as tests/path_step_child.py is."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "path_step_list_child.py")
    run = subprocess.run([sys.executable, child, prec], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "path_step_list_into ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
