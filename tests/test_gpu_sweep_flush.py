"""GPU parity for the flush stage of the general sweep's per-lane exact tests (rt_sweep.hpp, nearest_hit: flush).
The fp32 scene-frame kernels work off each lane's candidates of a cluster pair after the pair's last walked
cluster, one sphere per step, gathering the sphere from the flat slot table (rt_layout.hpp, pack_flat: one
{cx, cy, cz, r^2} record per slot, the scene index from ridx at the same slot).  The scenes aim at what the
gather and the flush scope can get wrong: single rays with candidates in every cluster pair of several supers,
lanes with every bit of their word set next to lanes with none, equal-t hits whose tie is broken across flushes
of different pairs and supers, every slot a candidate (RT_FILTER_OFF=1), the last super of the largest scene the
non-mega kernels take (the end of the table), one cluster alone, padding slots, and waves with few live lanes;
every case in every mode that shares the path (V2, ROOT2, scalar, v1, v3) and through the split, window and
items kernels (CASES).  They hold as they are for a
flush that is deferred across pairs or supers.

Bar: the linear image array_equal, the RGB8 bytes equal, ray_segments and the return code equal to the CPU
oracle's (0 ulp).  Every camera has a defocus disk, so the primary rays take the general sweep too.  Frames are at
most 16x16 at 8 spp, depth at most 6; fp32 only (fp64 rays and the mega kernels keep the wave-level exact tests,
tests/test_gpu_lane_exact.py).
"""
import numpy as np
import pytest

import edge_scenes as es
import rt_mi355x as rt
from rt_mi355x import abi
from oracle_bind import oracle_render

pytestmark = pytest.mark.gpu

SEED = es.SEED
F32 = abi.RT_FLAG_F32
SCALAR = abi.RT_FLAG_MODE_SCALAR
# every mode that instantiates the general sweep: V2 (the live path), both roots, scalar, v1 and v3
MODES = [0, abi.RT_FLAG_ROOT2, SCALAR, abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_VECTORIZED3]


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    monkeypatch.delenv("RT_FILTER_OFF", raising=False)
    monkeypatch.delenv("RT_WAVES", raising=False)


# ---------------------------------------------------------------- scenes
GROUND = ((0.0, -1000.0, 0.0), 1000.0, rt.Lambertian((0.5, 0.5, 0.5)))
AXIS_CAMERA = dict(rt.MAIN_CAMERA, center=(0.0, 1.0, 6.0), look_at=(0.0, 1.0, 0.0), focal_length=6.0,
                   view_angle=40.0, defocus_angle=0.6)


def _flat(objs):
    return rt.FlatScene(np.array([o[0] for o in objs], dtype=np.float64), np.array([o[1] for o in objs], dtype=np.float64),
                        np.arange(len(objs), dtype=np.uint32), [o[2] for o in objs])


def _glassy(rng, n):
    """Mostly glass, so paths run on through the spheres behind; the rest mixed."""
    return [rt.Dielectric(1.5, False) if rng.random() < 0.6 else m for m in es._mixed(rng, n)]


_scenes = {}


def _cached(key, build):
    if key not in _scenes:
        _scenes[key] = build()
    return _scenes[key]


def row(n=200, w=16, h=8):
    """n overlapping spheres of radius 0.25 on the line (0, 1, -0.3 k), seen along the line: the k-d splits cut the
    row into runs of 16 (a cluster), 64 (a super) in z order, n = 200 gives 13 clusters in 4 supers.  A ray down
    the axis passes the filter of every sphere of the row, so it holds candidates in every cluster pair of every
    super (a flush that kept candidates pending would meet a conflict at each walked pair after the first).  Rays
    off the axis pass a few pairs or none."""
    def build():
        rng = np.random.default_rng(2000 + n)
        objs = [((0.0, 1.0, -0.3 * k), 0.25, m) for k, m in enumerate(_glassy(rng, n))]
        objs.append(GROUND)
        return _flat(objs)
    return _cached(("row", n), build), rt.camera_new_py(w, h, **AXIS_CAMERA)


def shells(n, w=16, h=8):
    """n concentric shells at (0, 1, 0), radii 1 .. 1.5 shuffled (none always-exact).  Equal centres: the slots follow
    the scene order, 64 fill the four clusters of one super, 80 spill into a second.  An axis lane has all 16 bits of
    every cluster set (32 candidates per word), a lane past the outermost shell none."""
    def build():
        rng = np.random.default_rng(7000 + n)
        r = 1.0 + 0.5 * rng.permutation(n) / max(n - 1, 1)
        mats = _glassy(rng, n)
        return _flat([((0.0, 1.0, 0.0), r[k], mats[k]) for k in range(n)] + [GROUND])
    return _cached(("shells", n), build), rt.camera_new_py(w, h, **AXIS_CAMERA)


def identical(n=80, w=16, h=8):
    """The ground, then n identical spheres at (0, 1, 0): slot order is scene order, so one equal-t tie spans the
    clusters of a super and two supers; the later scene index wins (scalar mode: the earlier), whichever flush
    brings each of them in."""
    def build():
        rng = np.random.default_rng(900 + n)
        return _flat([GROUND] + [((0.0, 1.0, 0.0), 1.0, rt.Lambertian(tuple(rng.uniform(0.05, 0.95, 3))))
                                 for _ in range(n)])
    return _cached(("identical", n), build), rt.camera_new_py(w, h, **AXIS_CAMERA)


def slab(n, w=16, h=16):
    """n spheres of radius 0.2 .. 0.3 in a slab around y = 1 plus the ground.  n = 2048 fills 128 clusters, 32
    supers: the largest scene the non-mega kernels take (super index 31, the last records of the flat table)."""
    def build():
        rng = np.random.default_rng(3000 + n)
        c = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([16.0, 0.6, 16.0]) + np.array([0.0, 1.0, 0.0])
        r = rng.uniform(0.2, 0.3, n)
        mats = es._mixed(rng, n)
        return _flat([(tuple(c[k]), float(r[k]), mats[k]) for k in range(n)] + [GROUND])
    cam = dict(AXIS_CAMERA, center=(0.0, 4.0, 24.0), look_at=(0.0, 1.0, 0.0), focal_length=24.0, view_angle=60.0,
               defocus_angle=0.4)
    return _cached(("slab", n), build), rt.camera_new_py(w, h, **cam)


def counted(n, w=16, h=8):
    """edge_scenes.count(n) plus a ground under a defocus camera: 16 - n % 16 padding slots in the last cluster and
    whole padding clusters up to a multiple of 4.  A dummy slot is never a candidate and never hit."""
    def build():
        base, _ = es.count(n)
        objs = [(tuple(base.center[k]), float(base.radius[k]), base.materials[int(base.material[k])]) for k in range(n)]
        return _flat(objs + [GROUND])
    cam = dict(AXIS_CAMERA, center=(0.0, 1.5, 7.0), focal_length=7.0, defocus_angle=0.4)
    return _cached(("counted", n), build), rt.camera_new_py(w, h, **cam)


# ---------------------------------------------------------------- the bar
_refs = {}


def reference(key, flat, cam, depth, spp, flags):
    """oracle_render, once per key, read-only."""
    if key not in _refs:
        r = oracle_render(flat, cam, depth, spp, SEED, flags & ~F32, precision="f32")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def assert_equal_to_oracle(got, key, scene, flags, spp, depth):
    flat, cam = scene
    rgb_g, lin_g, st, rc_g = got
    rgb_o, lin_o, segs_o, rc_o = reference((key, flags, spp, depth), flat, cam, depth, spp, flags)
    assert rc_g == rc_o
    diff = np.argwhere(lin_g != lin_o)
    assert diff.size == 0, (
        f"{len(diff)} mismatching channels of {lin_o.size}; first pixel {diff[0][0]}: gpu {lin_g[diff[0][0]]} "
        f"oracle {lin_o[diff[0][0]]}")
    np.testing.assert_array_equal(rgb_g, rgb_o)
    return st, segs_o


def assert_parity(renderer, key, scene, flags, spp=8, depth=4, samples_per_item=None):
    flat, cam = scene
    renderer.seed, renderer.flags = SEED, F32 | flags
    got = renderer.render_flat(depth, spp, flat, cam, want_linear=True, samples_per_item=samples_per_item)
    st, segs_o = assert_equal_to_oracle(got, key, scene, flags, spp, depth)
    assert st.ray_segments == segs_o
    assert st.samples == cam.image_width * cam.image_height * spp
    assert st.exact_tests > 0 and st.filter_groups > 0
    k = abi.kernel_info(st.kernel_id)
    assert k["T"] == "float" and not k["mega"]
    return got[1], st


# ---------------------------------------------------------------- the cases
# name -> (key of the oracle reference, scene, spp, depth, RT_FILTER_OFF).  STRUCTURE: what build_layout must make of
# each scene for the case to reach what it is about (n_top supers, n_xs always-exact spheres, n_mg mega groups);
# tests/test_flat_slots.py checks it on the host, so a drift of the layout's heuristics fails there.
CASES = {
    # single rays with candidates in every cluster pair of four supers
    "row": ("row", row, 8, 6, False),
    # all 32 bits of both words of one super for the axis lanes, none for the lanes that miss; 80: a second super
    "shells64": (("shells", 64), lambda: shells(64), 8, 4, False),
    "shells80": (("shells", 80), lambda: shells(80), 8, 4, False),
    # one equal-t tie across the clusters of a super and two supers
    "identical": ("identical", identical, 8, 4, False),
    # RT_FILTER_OFF=1: every real sphere of every walked cluster is a candidate of every lane
    "row_off": (("row", 8, 8), lambda: row(w=8, h=8), 4, 4, True),
    "shells_off": (("shells", 80, 8, 8), lambda: shells(80, w=8, h=8), 4, 4, True),
    # 2048 filtered spheres: 32 supers, the last at the end of the flat table; still the non-mega kernels
    "slab2048": ("slab2048", lambda: slab(2048), 2, 4, False),
    # one cluster (one super, three padding clusters)
    "single": (("shells", 16), lambda: shells(16), 8, 4, False),
    # 5x3 at 3 spp: 45 samples, one wave with 19 idle lanes
    "partial": (("row", 5, 3), lambda: row(w=5, h=3), 3, 4, False),
    # padding slots in the last cluster, whole padding clusters
    "counted5": (("counted", 5), lambda: counted(5), 8, 4, False),
    "counted17": (("counted", 17), lambda: counted(17), 8, 4, False),
    "counted65": (("counted", 65), lambda: counted(65), 8, 4, False),
}
STRUCTURE = {   # case -> (n_top, n_xs, n_mg)
    "row": (4, 1, 0), "shells64": (1, 1, 0), "shells80": (2, 1, 0), "identical": (2, 1, 0), "row_off": (4, 1, 0),
    "shells_off": (2, 1, 0), "slab2048": (32, 1, 0), "single": (1, 1, 0), "partial": (4, 1, 0),
    "counted5": (1, 1, 0), "counted17": (1, 1, 0), "counted65": (2, 1, 0),
}


def _case(name, monkeypatch):
    key, build, spp, depth, off = CASES[name]
    if off:
        monkeypatch.setenv("RT_FILTER_OFF", "1")
    return key, build(), spp, depth


# ---------------------------------------------------------------- every case in every mode
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_modes(renderer, name, mode, monkeypatch):
    key, scene, spp, depth = _case(name, monkeypatch)
    assert_parity(renderer, key, scene, mode, spp=spp, depth=depth)


@pytest.mark.parametrize("depth", [1, 2])
def test_two_super_candidates_depths(renderer, depth):
    """Depth 1: the primary rays alone, aimed down the row from the defocus disk.  Depth 2: one bounce from inside it."""
    assert_parity(renderer, "row", row(), 0, depth=depth)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["row_off", "shells_off"])
def test_filter_off_is_the_filtered_image(renderer, name, mode, monkeypatch):
    """The same image with and without the filter (both the oracle's), and no fewer exact tests without it."""
    key, build, spp, depth, _ = CASES[name]
    lin_f, st_f = assert_parity(renderer, key, build(), mode, spp=spp, depth=depth)
    monkeypatch.setenv("RT_FILTER_OFF", "1")
    lin_x, st_x = assert_parity(renderer, key, build(), mode, spp=spp, depth=depth)
    np.testing.assert_array_equal(lin_f, lin_x)
    assert st_x.exact_tests >= st_f.exact_tests > 0


# ---------------------------------------------------------------- every case through the split, window and items kernels
@pytest.mark.parametrize("name", list(CASES))
def test_split_kernel(renderer, name, monkeypatch):
    """The sample-parallel kernel, half the samples per item (two or three items per pixel)."""
    key, scene, spp, depth = _case(name, monkeypatch)
    _, st = assert_parity(renderer, key, scene, 0, spp=spp, depth=depth, samples_per_item=max(1, spp // 2))
    assert abi.RT_KERNEL_SPLIT(st.kernel_id)


@pytest.mark.parametrize("name", list(CASES))
def test_window_and_items_kernels(renderer, name, monkeypatch):
    """A progressive session: half the samples, then all (trace_paths_window); then per-pixel counts, half or all,
    from a second session (trace_paths_items).  Every image is the one-launch render's at that count."""
    key, scene, spp, depth = _case(name, monkeypatch)
    flat, cam = scene
    half = max(1, spp // 2)
    renderer.seed, renderer.flags = SEED, F32
    with renderer.begin_progressive(depth, spp, flat, cam) as s:
        assert_equal_to_oracle(s.extend(half, want_linear=True), key, scene, 0, half, depth)
        st, _ = assert_equal_to_oracle(s.extend(spp, want_linear=True), key, scene, 0, spp, depth)
        assert st.exact_tests > 0
    npx = cam.image_width * cam.image_height
    targets = np.where(np.arange(npx) % 3 == 0, spp, half).astype(np.uint32)
    with renderer.begin_progressive(depth, spp, flat, cam) as s:
        rgb, lin, st, rc = s.extend_map(targets, want_linear=True)
        assert st.exact_tests > 0 and abi.RT_KERNEL_ITEMS(st.kernel_id)
    _, lin_h, _, _ = reference((key, 0, half, depth), flat, cam, depth, half, 0)
    _, lin_a, _, _ = reference((key, 0, spp, depth), flat, cam, depth, spp, 0)
    np.testing.assert_array_equal(lin, np.where((targets == spp)[:, None], lin_a, lin_h))


# ---------------------------------------------------------------- the counter
def test_exact_tests_counter(renderer):
    """One count per wave step: positive with the filter, and no smaller with every slot a candidate (checked in
    test_filter_off_is_the_filtered_image); a sweep that walks nothing counts the always-exact group alone."""
    _, st = assert_parity(renderer, "row", row(), 0, depth=6)
    sweeps_floor = st.ray_segments // 64   # at least this many wave sweeps (64 lanes each), 2 exact tests each
    assert st.exact_tests >= 2 * sweeps_floor
