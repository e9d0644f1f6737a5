"""The sweeps' culls on the device, against brute force: the adversarial rays of tests/cull_cases.py (their shares are
checked on the CPU in tests/test_cull_cases.py) through the product's own nearest_hit and camera_sweep
(tests/device/rt_devunit.hip's ray probe, over the tables build_scene_image makes), compared with
oracle_nearest_hit, which tests every sphere in scene order with the reference's arithmetic and no cull.  The bar is
the project's usual one: the same index and the same bits of t for every active lane, and inactive lanes untouched.

A cull that drops a sphere the reference could hit shows here as a lane that misses (or reports a farther sphere)
where the oracle hits; the solo composition (one active lane per wave) is the one in which no neighbouring lane can
pass the box, the group or the cone on the lane's behalf.  The controls say where to look when something fails: the
same rays with the filters off (f_cmax = +inf, pass_all), and plain random rays, must match too, and a failure there
points at the probe's table wiring, not at a cull.
"""
import numpy as np
import pytest

import cull_cases as cc
import devunit_bind as db

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(cc.SCENES)
PRECS = list(cc.DTYPES)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(sc, la, mode, got, what):
    """None, or the report of the first lanes whose (index, t) differs from the oracle's: lane in its wave, the
    case's target and measured delta, what the probe and the oracle say."""
    want_i, want_t = cc.reference(sc, mode, la.rays, la.active)
    got_i, got_t = got
    bad = np.flatnonzero((got_i != want_i) | (_bits(got_t) != _bits(want_t)))
    if bad.size == 0:
        return None
    rows = []
    for i in bad[:6]:
        rows.append(f"ray {i} (wave {i // 64} lane {i % 64}, {'active' if la.active[i] else 'inactive'}): target "
                    f"{la.rays.target[i]} delta {la.rays.delta[i]:.3e}; probe ({got_i[i]}, {got_t[i]!r} "
                    f"{got_t[i:i + 1].tobytes().hex()}), oracle ({want_i[i]}, {want_t[i]!r} {want_t[i:i + 1].tobytes().hex()}); "
                    f"o {la.rays.o[:, i].tolist()} d {la.rays.d[:, i].tolist()}")
    lost = int(((want_i >= 0) & (got_i != want_i))[bad].sum())
    return f"{what} [{mode}]: {bad.size} of {int(la.active.sum())} active lanes differ ({lost} with an oracle hit); " + "; ".join(rows)


def probe(sc, la, mode, filter_off=False):
    if la.rays.centre is not None:
        return db.probe_camera(sc.flat, mode, la.rays.centre, la.rays.d, la.active, filter_off)
    return db.probe_general(sc.flat, mode, la.rays.o, la.rays.d, la.active, filter_off)


def run_all_modes(sc, la, what, filter_off=False):
    reports = [check(sc, la, mode, probe(sc, la, mode, filter_off), what) for mode in cc.MODES]
    reports = [r for r in reports if r]
    assert not reports, "\n".join(reports)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", cc.COMPOSITIONS)
@pytest.mark.parametrize("fam", cc.GENERAL_FAMILIES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_general_sweep(name, fam, kind, prec):
    """nearest_hit: the fp32 distance filter and its per-lane constants (graze), the cluster, super, mega and giga slab
    tests with the best-hit bound (box_graze; near_equal: two spheres of different clusters within an ulp of each
    other, the bound against the tie rule), the zero basis and the clamps (degenerate)."""
    sc = cc.scene(name)
    la = cc.compose(sc, fam, cc.DTYPES[prec], kind)
    run_all_modes(sc, la, f"{name}/{fam}/{kind}/{prec}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", cc.CAMERA_COMPOSITIONS)
@pytest.mark.parametrize("fam", cc.CAMERA_FAMILIES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_camera_sweep(name, fam, kind, prec):
    """camera_sweep / cone_walk over build_cam_table's rp records, from a centre outside every sphere (two of them),
    inside one and on one: a single valid lane, a narrow cone, a spread beyond 60 degrees, and grazing lanes beside
    degenerate and missing ones."""
    sc = cc.scene(name)
    la = cc.compose(sc, fam, cc.DTYPES[prec], kind)
    run_all_modes(sc, la, f"{name}/{fam}/{kind}/{prec}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_control_general(name, prec):
    """The probe's wiring: every family's rays with the filters off, and 4096 plain random rays with them on and off."""
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    for fam in cc.GENERAL_FAMILIES:
        la = cc.compose(sc, fam, dtype, "full")
        run_all_modes(sc, la, f"{name}/{fam}/full/{prec}/filter_off", filter_off=True)
    rays = cc.random_rays(sc, dtype)
    la = cc.Launch(rays, np.ones(rays.n, np.uint8), np.full(rays.n, -1))
    hit, _ = cc.reference(sc, "packed", rays)
    assert 0.2 < (hit >= 0).mean() < 1.0 and np.unique(hit).size > min(30, sc.flat.n_spheres // 2)   # the control sees the scene
    run_all_modes(sc, la, f"{name}/random/{prec}")
    run_all_modes(sc, la, f"{name}/random/{prec}/filter_off", filter_off=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_control_camera(name, prec):
    """The same from each camera centre: the grazing rays with pass_all, and 4096 random directions."""
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    for fam in cc.CAMERA_FAMILIES:
        la = cc.compose(sc, fam, dtype, "full")
        run_all_modes(sc, la, f"{name}/{fam}/full/{prec}/filter_off", filter_off=True)
        P = la.rays.centre
        rnd = cc.random_rays(sc, dtype)
        rays = cc.Rays(np.repeat(P[:, None], rnd.n, 1), rnd.d, centre=P)
        lr = cc.Launch(rays, np.ones(rays.n, np.uint8), np.full(rays.n, -1))
        run_all_modes(sc, lr, f"{name}/{fam}/random/{prec}")
        run_all_modes(sc, lr, f"{name}/{fam}/random/{prec}/filter_off", filter_off=True)
