"""GPU parity for the general sweep's exact tests behind the sphere filter (rt_sweep.hpp, nearest_hit): the
fp32 non-mega kernels keep, per lane, a 16-bit mask of the lane's own passing spheres in a walked cluster and
work it off one sphere per step after the cluster's 4 filter groups; fp64 rays and the mega kernels test the
sphere pairs / spheres that any lane passes.  The scenes aim at what either scheme can get wrong: a lane with
every slot of a cluster set next to lanes with none, the first and the last slot of a cluster, candidates in
several clusters and supers, ties across pairs, groups, clusters and supers, padding slots, waves with few
live lanes, and lanes whose filter passes everything.

Bar: the linear image array_equal, the RGB8 bytes equal, ray_segments and the return code equal to the CPU
oracle's (0 ulp).  Every camera but the last test's has a defocus disk, so the primary rays take the general
sweep too and can be aimed.  Frames are at most 16x8 at 8 spp, depth 1 .. 4.
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
# every mode that instantiates the general sweep: the live path, both roots, and the two semantics modes
MODES = [0, abi.RT_FLAG_ROOT2, SCALAR, abi.RT_FLAG_MODE_VECTORIZED]
PRECS = [F32, 0]


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    monkeypatch.delenv("RT_FILTER_OFF", raising=False)
    monkeypatch.delenv("RT_WAVES", raising=False)


# ---------------------------------------------------------------- scenes
GROUND = ((0.0, -1000.0, 0.0), 1000.0, rt.Lambertian((0.5, 0.5, 0.5)))
# looks along -z at (0, 1, 0) from 6 units away; the disk makes every primary ray a general-sweep ray
AXIS_CAMERA = dict(rt.MAIN_CAMERA, center=(0.0, 1.0, 6.0), look_at=(0.0, 1.0, 0.0), focal_length=6.0,
                   view_angle=40.0, defocus_angle=0.6)


def _flat(objs):
    return rt.FlatScene(np.array([o[0] for o in objs], dtype=np.float64), np.array([o[1] for o in objs], dtype=np.float64),
                        np.arange(len(objs), dtype=np.uint32), [o[2] for o in objs])


def _shell_materials(rng, n):
    """Mostly glass, so paths cross many shells and leave again; the rest mixed."""
    return [rt.Dielectric(1.5, False) if rng.random() < 0.6 else m for m in es._mixed(rng, n)]


def nested(n, ground=True, w=16, h=8):
    """n shells at (0, 1, 0), radii 1 .. 1.5 in a shuffled order (all within 3x of the median radius, so none joins
    the always-exact group).  Equal centres: the k-d splits rest on the scene index, so the slots of the clusters
    follow the scene order: n = 16 fills one cluster, 64 one super of 4 clusters, 80 splits 64 | 16 into two
    supers.  A ray along the view axis passes the filter of every shell (all n slots of its masks set), a ray
    past the outermost shell passes none, and the rays in between pass the outer shells only, wherever the
    shuffle put them."""
    rng = np.random.default_rng(7000 + n)
    r = 1.0 + 0.5 * rng.permutation(n) / max(n - 1, 1)
    mats = _shell_materials(rng, n)
    objs = [((0.0, 1.0, 0.0), r[k], mats[k]) for k in range(n)]
    if ground:
        objs.append(GROUND)
    return _flat(objs), rt.camera_new_py(w, h, **AXIS_CAMERA)


def first_last(w=16, h=8):
    """16 spheres in a row along x, one cluster whose slot order is the order of x (kd_order), seen from the
    front: a primary ray passes the filter of the one or two spheres in front of it, so the lanes of a wave hold
    single candidates at different slots, the first and the last slot of the mask among them (the mirror
    spheres at both ends), and the sky lanes above the row none."""
    rng = np.random.default_rng(16)
    objs = [((0.5 * (k - 7.5), 1.0, 0.0), 0.24, rt.Metal((0.9, 0.9, 0.9), 0.0) if k in (0, 15) else m)
            for k, m in enumerate(es._mixed(rng, 16))]
    objs.append(GROUND)
    cam = dict(AXIS_CAMERA, center=(0.0, 1.0, 9.0), focal_length=9.0, view_angle=52.0, defocus_angle=0.3)
    return _flat(objs), rt.camera_new_py(w, h, **cam)


def copies(n, adjacent, w=16, h=8):
    """Ties.  adjacent: 8 separate spheres, each twice at scene indices 2k, 2k + 1 with different materials: the
    copies share a centre, so the index tie-break keeps them next to each other through kd_order and they share
    an exact pair.  Otherwise n identical spheres at (0, 1, 0) after the ground: slot order is scene order, so
    one tie spans the pairs and groups of a cluster (n = 16), clusters (n = 40) and supers (n = 80); the later
    scene index wins (scalar mode: the earlier)."""
    rng = np.random.default_rng(900 + n)
    if adjacent:
        objs = []
        for k, m in enumerate(es._mixed(rng, 8)):
            c = (1.1 * (k % 4 - 1.5), 0.6 + 1.0 * (k // 4), 0.0)
            objs += [(c, 0.5, m), (c, 0.5, es._other_material(m))]
        objs.append(GROUND)
    else:
        objs = [GROUND] + [((0.0, 1.0, 0.0), 1.0, rt.Lambertian(tuple(rng.uniform(0.05, 0.95, 3)))) for _ in range(n)]
    return _flat(objs), rt.camera_new_py(w, h, **AXIS_CAMERA)


def counted(n, w=16, h=8):
    """edge_scenes.count(n) plus a ground, under a defocus camera: n filtered spheres leave 16 - n % 16 padding
    slots in the last cluster (and whole padding clusters up to a multiple of 4).  A dummy slot is never a
    candidate and never hit."""
    base, _ = es.count(n)
    objs = [(tuple(base.center[k]), float(base.radius[k]), base.materials[int(base.material[k])]) for k in range(n)]
    objs.append(GROUND)
    cam = dict(AXIS_CAMERA, center=(0.0, 1.5, 7.0), focal_length=7.0, defocus_angle=0.4)
    return _flat(objs), rt.camera_new_py(w, h, **cam)


# ---------------------------------------------------------------- the bar
_refs = {}


def reference(key, flat, cam, depth, spp, flags):
    """oracle_render, once per key, read-only."""
    if key not in _refs:
        r = oracle_render(flat, cam, depth, spp, SEED, flags & ~F32, precision="f32" if flags & F32 else "f64")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def assert_parity(renderer, key, scene, flags, spp=8, depth=4):
    flat, cam = scene
    renderer.seed, renderer.flags = SEED, flags
    rgb_g, lin_g, st, rc_g = renderer.render_flat(depth, spp, flat, cam, want_linear=True)
    rgb_o, lin_o, segs_o, rc_o = reference((key, flags, spp, depth), flat, cam, depth, spp, flags)
    assert rc_g == rc_o
    diff = np.argwhere(lin_g != lin_o)
    assert diff.size == 0, (
        f"{len(diff)} mismatching channels of {lin_o.size}; first pixel {diff[0][0]}: gpu {lin_g[diff[0][0]]} "
        f"oracle {lin_o[diff[0][0]]}")
    np.testing.assert_array_equal(rgb_g, rgb_o)
    assert st.ray_segments == segs_o
    assert st.samples == cam.image_width * cam.image_height * spp
    return lin_g, st


# ---------------------------------------------------------------- one lane, many candidates
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [16, 64, 80])
def test_nested(renderer, n, prec, mode):
    """16 shells: every bit of one cluster's mask for the axis lanes, none for the lanes that miss.  64: the four
    clusters of one super, each flushed before the next is filtered.  80: a second super after the first."""
    _, st = assert_parity(renderer, ("nested", n), nested(n), prec | mode)
    assert st.exact_tests > 0 and st.filter_groups > 0


@pytest.mark.parametrize("prec", PRECS)
def test_nested_no_ground(renderer, prec):
    """No always-exact sphere (n_xg = 0): the walked clusters' blocks start the filter stream."""
    assert_parity(renderer, ("nested_ng", 16), nested(16, ground=False), prec)


@pytest.mark.parametrize("depth", [1, 2])
def test_nested_depths(renderer, depth):
    """Depth 1: the primary rays alone, straight from the defocus disk.  Depth 2: one bounce from inside the shells."""
    assert_parity(renderer, ("nested", 80), nested(80), F32, depth=depth)


@pytest.mark.parametrize("mode", [0, SCALAR])
@pytest.mark.parametrize("prec", PRECS)
def test_first_and_last_slot(renderer, prec, mode):
    assert_parity(renderer, "first_last", first_last(), prec | mode)


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("where", ["pair", 16, 40, 80])
def test_ties(renderer, where, prec, mode):
    """The same sphere at two or more scene indices: in one exact pair, across the groups of a cluster (16),
    across clusters (40) and across supers (80)."""
    scene = copies(8, True) if where == "pair" else copies(where, False)
    assert_parity(renderer, ("copies", where), scene, prec | mode)


@pytest.mark.parametrize("mode", [0, SCALAR])
def test_ties_shared_generators(renderer, mode):
    """edge_scenes' own tie scenes under the fp32 kernels at this file's depth: twins (pairs inside clusters) and
    the 40-stack."""
    assert_parity(renderer, "es_twins", es.twins(100, 16, 8), F32 | mode)
    assert_parity(renderer, "es_stack", es.stack(16, 8), F32 | mode)


# ---------------------------------------------------------------- padding slots
@pytest.mark.parametrize("mode", [0, SCALAR])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 5, 17, 65])
def test_padding_slots(renderer, n, prec, mode):
    assert_parity(renderer, ("counted", n), counted(n), prec | mode)


# ---------------------------------------------------------------- few live lanes
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("w,h,spp", [(3, 3, 5), (5, 5, 7), (16, 8, 1)])
def test_partial_waves(renderer, w, h, spp, prec):
    """45 samples: one wave with 19 idle lanes.  175: the last batch holds 47.  128 at 1 spp: two full waves."""
    assert_parity(renderer, ("nested_wh", w, h), nested(16, w=w, h=h), prec, spp=spp)


# ---------------------------------------------------------------- every lane degenerate
@pytest.mark.parametrize("mode", [0, SCALAR])
@pytest.mark.parametrize("prec", PRECS)
def test_filter_off(renderer, prec, mode, monkeypatch):
    """RT_FILTER_OFF=1: every real sphere of every walked cluster is a candidate of every lane (16 steps per full
    cluster).  The same image as with the filter, and the oracle's."""
    scene = nested(80, w=8, h=8)
    lin_f, st_f = assert_parity(renderer, ("nested_off", 80), scene, prec | mode, spp=4)
    monkeypatch.setenv("RT_FILTER_OFF", "1")
    lin_x, st_x = assert_parity(renderer, ("nested_off", 80), scene, prec | mode, spp=4)
    np.testing.assert_array_equal(lin_f, lin_x)
    assert st_x.exact_tests >= st_f.exact_tests


# ---------------------------------------------------------------- the counter
def test_exact_tests_counter(renderer):
    """rt_stats.exact_tests counts the general sweep only: zero when a pinhole camera's primary rays (camera
    sweep) are all there is, positive once rays bounce."""
    flat, _ = nested(16)
    cam = rt.camera_new_py(16, 8, **dict(AXIS_CAMERA, defocus_angle=0.0))
    _, st1 = assert_parity(renderer, "pinhole", (flat, cam), F32, depth=1)
    assert st1.exact_tests == 0 and st1.filter_groups == 0 and st1.box_groups == 0
    _, st2 = assert_parity(renderer, "pinhole", (flat, cam), F32, depth=2)
    assert st2.exact_tests > 0 and st2.filter_groups > 0
