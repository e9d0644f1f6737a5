"""The device's next-ray stage on its own, at 0 ulp: the lanes of tests/scatter_cases.py (their conditions, a second
reference and the mutations they catch are checked on the CPU in tests/test_scatter_cases.py) through the product's
next_ray<T, SCALAR> (tests/device/rt_devunit.hip's next-ray probe, over the kernel arguments build_scene_image,
scene_params and frame_params make), compared with the oracle's next-ray and get-ray probes.

The bar is the project's usual one: the same bit patterns, signed zeros included (NaN where the reference is NaN), of
the hit point, the scattered direction and the colour of every scatter lane, of the origin and the direction of every
camera lane, whose colour is exactly 1, and idle lanes as the caller left them.  The camera and scatter lanes of one
wave share one Philox block, one sqrt_len and one dvs, so the mixed family also asks that every lane's result is the
one it has when the lanes of the other role are idle.
"""
import numpy as np
import pytest

import devunit_bind as db
import scatter_cases as sc
from device_math_cases import assert_bits, same_bits

pytestmark = pytest.mark.gpu

PRECS = list(sc.DTYPES)
ROLE_NAMES = {sc.IDLE: "idle", sc.CAMERA: "camera", sc.SCATTER: "scatter"}


def run(ln, la, mode):
    return db.next_ray(sc.table(), ln.cam, sc.SEED, mode, la.role, la.colx, la.rowy, la.pix, la.sid, la.k, la.hit_i,
                       la.hit_t, la.o, la.d, la.c)


def check(what, la, got, ref):
    """got against (o, d, c) of ref, per role and array, with the lane's inputs in the report."""
    for role, rname in ROLE_NAMES.items():
        at = np.flatnonzero(la.role == role)
        if at.size == 0:
            continue
        for name, g, r in zip(("o", "d", "c"), got, ref):
            inputs = (at, la.hit_i[at], la.hit_t[at], la.k[at], la.pix[at], la.sid[at], la.o[:, at], la.d[:, at])
            assert_bits(g[:, at], r[:, at], f"{what}: {name} of the {rname} lanes", inputs)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("fam", sc.FAMILIES)
def test_next_ray(fam, prec, mode):
    for ln, ref in zip(sc.family(fam, prec, mode), sc.family_reference(fam, prec, mode)):
        la = ln.lanes
        got = run(ln, la, mode)
        what = f"{ln.name}/{prec}/{mode}"
        check(what, la, got, (ref.o, ref.d, ref.c))
        cam = la.role == sc.CAMERA
        assert (got[2][:, cam] == 1.0).all() and not np.signbit(got[2][:, cam]).any(), what
        if fam == "mixed":
            # every lane alone with its own role: the other role's lanes idle, in the same places
            for keep in (sc.SCATTER, sc.CAMERA):
                solo = la.with_roles(keep)
                if not (solo.role == keep).any():
                    continue
                alone = run(ln, solo, mode)
                at = np.flatnonzero(la.role == keep)
                for name, g, a in zip(("o", "d", "c"), got, alone):
                    assert_bits(g[:, at], a[:, at], f"{what}: {name} of the {ROLE_NAMES[keep]} lanes, mixed against alone",
                                (at,))
                off = solo.role == sc.IDLE
                for g, src in zip(alone, (solo.o, solo.d, solo.c)):
                    assert same_bits(g[:, off], src[:, off]).all(), f"{what}: an idle lane was written"
