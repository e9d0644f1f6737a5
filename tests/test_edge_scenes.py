"""The scenes of tests/edge_scenes.py do, on the CPU oracle alone, what tests/test_gpu_scene_edges.py needs them
for: a GPU parity test on a scene whose twins never tie in view, whose negative spheres are out of frame or
whose rays all sit on one side of a threshold would pass without reaching the branch it is named for.

Every share below is a floor the INPUT must clear on the oracle (measured values in the docstrings); none is a
measurement of the kernels.  The second half pins the oracle itself on the three scenes whose behaviour no
other test of the oracle covers (ties far apart in scene order, signed and zero radii, the material table's
extremes) against the independent restatement, tests/independent_v2.py, bit for bit.
"""
import ctypes

import numpy as np
import pytest

import edge_scenes as es
import independent_v2 as iv
import rt_mi355x as rt
from rt_mi355x import abi
from oracle_bind import load_oracle, oracle_render

SEED = es.SEED
SCALAR = abi.RT_FLAG_MODE_SCALAR
ROOT2 = abi.RT_FLAG_ROOT2
PRECS = ["f64", "f32"]


def render(scene, flags=0, prec="f64", spp=8, depth=50):
    """oracle_render of a (flat, cam) pair: the linear image and the segment count; rc 0, no NaN."""
    flat, cam = scene
    _, lin, segs, rc = oracle_render(flat, cam, depth, spp, SEED, flags, precision=prec)
    assert rc == 0
    assert not np.isnan(lin).any()
    return lin, segs


def changed(a, b):
    """Share of pixels that differ in any channel."""
    return float((a != b).any(axis=1).mean())


def empty_like(cam):
    return rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32), [rt.Lambertian((0.5, 0.5, 0.5))]), cam


# ---------------------------------------------------------------- the floors
@pytest.mark.parametrize("prec", PRECS)
def test_twins_tie_in_view(prec):
    """Exchanging the materials inside every pair changes the image where a twin pair is the nearest hit, and
    only there (the geometry is the same): at least half of the pixels.  Measured at 16x9: 63 % (f64), 65 %
    (f32), every pixel that is not sky (the ground is twinned too)."""
    a, _ = render(es.twins(), prec=prec)
    b, _ = render(es.twins(swap=True), prec=prec)
    assert changed(a, b) >= 0.5


@pytest.mark.parametrize("prec", PRECS)
def test_twins_mega_renders(prec):
    a, segs = render(es.twins_mega(), prec=prec, spp=16)
    b, _ = render(es.twins_mega(swap=True), prec=prec, spp=16)
    assert changed(a, b) >= 0.5 and segs > 8 * 5 * 16


@pytest.mark.parametrize("flags", [0, SCALAR])
@pytest.mark.parametrize("prec", PRECS)
def test_stack_ties_in_view(prec, flags):
    """Reversing the 40 materials changes which albedo the stack shows (the last sphere's on the packed paths,
    objects.rs:141; the first's in scalar mode): at least 10 % of the pixels.  Measured 61 % (f64), 63 % (f32)
    on both paths, with the camera 4 units from the stack."""
    a, _ = render(es.stack(), flags, prec)
    b, _ = render(es.stack(reverse=True), flags, prec)
    assert changed(a, b) >= 0.1


@pytest.mark.parametrize("prec", PRECS)
def test_radii_signs_in_view(prec):
    """Scalar mode divides by the signed radius (objects.rs:242), so |r| for r changes at least 10 % of the
    pixels (measured 22 % f64, 24 % f32).  The packed paths see r only as r.powi(2) (objects.rs:256) and take the
    normal from the hit itself: |r| changes nothing there, with or without ROOT2 (0 %, asserted exactly)."""
    a, _ = render(es.radii(), SCALAR, prec)
    b, _ = render(es.radii(absolute=True), SCALAR, prec)
    assert changed(a, b) >= 0.1
    for flags in (0, ROOT2):
        a, sa = render(es.radii(), flags, prec)
        b, sb = render(es.radii(absolute=True), flags, prec)
        np.testing.assert_array_equal(a, b)
        assert sa == sb


@pytest.mark.parametrize("prec", PRECS)
def test_materials_in_view(prec):
    """Every one of the 11 extreme spheres is some pixel's first hit: removing it changes the image."""
    flat, cam = es.materials(24, 14)
    a, segs = render((flat, cam), prec=prec)
    assert segs > 24 * 14 * 8
    for k in range(1, 12):
        keep = [i for i in range(12) if i != k]
        less = rt.FlatScene(flat.center[keep], flat.radius[keep], flat.material[keep], flat.materials)
        b, _ = render((less, cam), prec=prec)
        assert changed(a, b) > 0, k


def primary_L(cam, spp=8):
    """fx^2 + fz^2 in fp32 of every primary direction (oracle_get_ray_f64), as nearest_hit computes its L."""
    lib = load_oracle()
    o, d = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
    out = []
    for row in range(cam.image_height):
        for col in range(cam.image_width):
            for s in range(spp):
                lib.oracle_get_ray_f64(ctypes.addressof(cam), col, row, s, SEED, o, d)
                fx, fz = np.float32(d[0]), np.float32(d[2])
                out.append(fx * fx + fz * fz)
    return np.array(out, dtype=np.float32)


def test_needle_straddles_the_basis_threshold():
    """nearest_hit zeroes a lane's filter basis when L = fx^2 + fz^2 < 1e-15 (rt_sweep.hpp:417).  down_1e-6 has
    at least 5 % of its primary rays on each side (measured on the 48x3 strip: 22 % below, min 2.9e-18, max
    1.9e-14; a 16x9 frame at this view angle stays below 3.1e-16, all on one side); down_1e-30 has all below."""
    _, cam = es.needle("down_1e-6")
    L = primary_L(cam)
    below = float((L < np.float32(1e-15)).mean())
    assert below >= 0.05 and 1.0 - below >= 0.05, (below, L.min(), L.max())
    _, cam = es.needle("down_1e-30")
    assert (primary_L(cam) < np.float32(1e-15)).all()
    # along_x: the y and z components of every direction are below inv_ax's clamp, 1e-20 (rt_sweep.hpp:410-412)
    _, cam = es.needle("along_x")
    lib = load_oracle()
    o, d = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
    for col, row, s in [(0, 0, 0), (47, 2, 7), (20, 1, 3)]:
        lib.oracle_get_ray_f64(ctypes.addressof(cam), col, row, s, SEED, o, d)
        assert d[0] == 1.0 and abs(np.float32(d[1])) < 1e-20 and abs(np.float32(d[2])) < 1e-20


@pytest.mark.parametrize("kind", es.NEEDLES)
@pytest.mark.parametrize("prec", PRECS)
def test_needles_hit_something(kind, prec):
    flat, cam = es.needle(kind)
    _, segs = render((flat, cam), prec=prec)
    assert segs > cam.image_width * cam.image_height * 8
    render((flat, cam), SCALAR, prec)


@pytest.mark.parametrize("s", es.SCALES)
def test_scaled_f64_sees_the_scene(s):
    """fp64 has the range for every scale: at least 30 % of the pixels differ from the empty scene's (measured
    59.5 % at 24x14 at every scale)."""
    a, _ = render(es.scaled(s))
    b, _ = render(es.scaled(s, empty=True))
    assert changed(a, b) >= 0.3
    render(es.scaled(s), SCALAR)


@pytest.mark.parametrize("s", es.SCALES)
def test_scaled_f32_sees_the_scene_up_to_1e16(s):
    """fp32: the same floor up to 1e16 (59.5 %).  At 1e19 and 1e25 the squares of fp32 coordinates overflow, every
    discriminant is inf - inf or -inf, and the oracle renders pure sky with exactly one segment per sample: the
    GPU must agree with that too."""
    a, segs = render(es.scaled(s), prec="f32")
    b, _ = render(es.scaled(s, empty=True), prec="f32")
    if s <= 1e16:
        assert changed(a, b) >= 0.3
    else:
        np.testing.assert_array_equal(a, b)
        assert segs == 24 * 14 * 8


@pytest.mark.parametrize("name", sorted(es.LAYOUT_FAMILIES))
@pytest.mark.parametrize("prec", PRECS)
def test_layout_families_in_view(name, prec):
    """At least 5 % of the pixels are not sky (measured: count1 and count2 lowest with 10 %, collinear 15 %)."""
    flat, cam = es.LAYOUT_FAMILIES[name]()
    a, _ = render((flat, cam), prec=prec)
    b, _ = render(empty_like(cam), prec=prec)
    assert changed(a, b) >= 0.05


def test_layout_families_are_what_they_say():
    """The statistics build_layout (rt_layout.hpp) branches on, restated: its "always exact" rule (|c|_1 + |r|
    above 8x the median) and its "big" rule (|r| above 3x the median radius of the rest, at most 8 of them)."""
    def groups(flat):
        key = np.abs(flat.center).sum(axis=1) + np.abs(flat.radius)
        med = np.sort(key)[len(key) // 2]
        exact = key > 8.0 * med
        rr = np.abs(flat.radius[~exact])
        big_ = np.zeros(len(key), bool)
        big_[~exact] = rr > 3.0 * np.sort(rr)[len(rr) // 2]
        return int(exact.sum()), int(big_.sum())
    assert groups(es.big(8)[0]) == (0, 8)        # 8 big spheres: the always-exact group holds exactly them
    assert groups(es.big(9)[0]) == (0, 9)        # 9 > kBigExact: they stay in the clusters, n_xs == 0
    assert groups(es.uniform()[0]) == (0, 0)     # n_xs == 0
    assert groups(es.concentric()[0]) == (0, 0)
    assert groups(es.stack()[0]) == (1, 0)       # the ground; 40 coincident spheres in 3 clusters
    assert groups(es.twins()[0]) == (2, 6)       # both grounds, then 2 x 3 big spheres
    for n in es.COUNTS:
        assert es.count(n)[0].n_spheres == n
    for f in (es.concentric, es.collinear, es.coplanar):
        c = f()[0].center
        assert (np.ptp(c, axis=0) == 0).sum() == {"concentric": 3, "collinear": 2, "coplanar": 1}[f.__name__]


# ---------------------------------------------------------------- the oracle's second pin on the new behaviour
def _independent(flat, kw, prec):
    W, H, spp, depth = 8, 5, 6, 50
    cam_abi = rt.camera_new_py(W, H, **kw)
    cam = iv.camera_new(W, H, kw["focal_length"], kw["view_angle"], kw["center"], kw["look_at"], kw["up"],
                        kw["defocus_angle"])
    lin, rgb, segs = iv.render(flat, cam, spp, depth, SEED, prec=prec)
    rgb_o, lin_o, segs_o, rc = oracle_render(flat, cam_abi, depth, spp, SEED, precision=prec)
    assert rc == 0 and segs == segs_o
    assert np.array_equal(np.array(lin, dtype=np.float64), lin_o)
    assert np.array_equal(np.array(rgb, dtype=np.uint8), rgb_o)


@pytest.mark.parametrize("prec", PRECS)
def test_twins_oracle_matches_independent(prec):
    """PackedHitRecords::update takes a hit with t <= best (objects.rs:141), so of two spheres with equal t the
    later in scene order wins: the oracle and the independent restatement agree bit for bit, segments included,
    on 100 pairs whose members are up to 199 indices apart."""
    _independent(es.twins()[0], es.TWINS_CAMERA, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_radii_oracle_matches_independent(prec):
    """Negative, zero and 1e-12 radii on the live path: hit_packed squares the radius (objects.rs:256) and never
    divides by it; the division by the signed radius is Sphere::hit's (objects.rs:242), scalar mode only, which
    the restatement does not cover.  The -r / +r pair ties (objects.rs:141)."""
    _independent(es.radii()[0], es.RADII_CAMERA, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_materials_oracle_matches_independent(prec):
    """Metal::new clamps fuzzy_factor only from above (materials.rs:79-88), so fuzz -0.5 stays and fuzz 1.0 is the
    largest; a hollow dielectric negates the normal before the refraction (materials.rs:131); ior 1, 0.7, 1e-3
    and 1e3 go through the same reflectance and refract arithmetic; albedo 0 and 1."""
    _independent(es.materials()[0], es.MATERIALS_CAMERA, prec)
