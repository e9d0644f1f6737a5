"""Guide buffers (guide_pixels<T, CAMQ, MEGA>, rt_guides.hpp) on the degenerate scenes of tests/edge_scenes.py and on
every path of the kernel that tests/test_gpu_guides.py leaves unreached.

The guide kernel runs the render kernels' culls with template arguments no render uses (camera_listed<T, false,
false> with a one-slot mask, camera_sweep<T, false, false, MEGA>, nearest_hit<T, false, false, MEGA> at
bounce 0 only) and its own copy of PackedHitRecords::finalize, and its outputs show what an image hides: the
hit index (albedo is the material of `hi`), the normal's sign, and t itself as float32.

Bar: test_gpu_guides's.  np.testing.assert_array_equal on the four float32 outputs against restate_guides, plus
check_stats: 0 ulp (NaN equal to NaN, as assert_array_equal has it).  tests/test_guide_edges.py holds the table
of cases (case(), samples(): one restatement per case and precision, shared) and shows on the restatement alone
that each scene reaches what it is here for.

Which path a pixel took is read from the statistics, never assumed: pixel_list walks the cone once per pixel,
camera_sweep once per batch, so a range has a pixel that fell back to the per-batch sweep exactly when its
cone_tests at 65 spp (two batches) exceed its cone_tests at 1 spp; for a listed pixel, camera_exact_tests of one
batch is the length of its list.
"""
import math

import numpy as np
import pytest

import edge_scenes as es
import independent_v2 as iv
from rt_mi355x import abi
from guide_restatement import fold, restate_guides
from test_gpu_guides import PRECS, assert_guides_equal, check_stats, guides
from test_guide_edges import case, cover_geometry, samples, tile_of

pytestmark = pytest.mark.gpu

GEOMETRY = ("normal", "depth", "coverage")


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    monkeypatch.delenv("RT_FILTER_OFF", raising=False)
    monkeypatch.delenv("RT_WAVES", raising=False)


def run(renderer, key, prec, spp=None, camq=True, mega=False):
    """The guides of case(key) at spp (None: the case's own count) against the restatement, with check_stats."""
    flat, cam, n, pixels = case(key)
    spp = n if spp is None else spp
    vals, _ = samples(key, prec)
    got, st = guides(renderer, prec, spp, flat, cam, tile=tile_of(key))
    assert_guides_equal(got, restate_guides(vals, spp))
    check_stats(st, cam.image_width * cam.image_height if pixels is None else len(pixels), spp, prec, camq=camq, mega=mega)
    return got, st


def cone_tests(renderer, key, prec, spp):
    flat, cam, _, _ = case(key)
    _, st = guides(renderer, prec, spp, flat, cam, tile=tile_of(key), want=("coverage",))
    return st.cone_tests


def fell_back(renderer, key, prec):
    """Some pixel of the case's range ran camera_sweep per batch (module docstring)."""
    one, two = cone_tests(renderer, key, prec, 1), cone_tests(renderer, key, prec, 65)
    assert two >= one
    return two > one


# ---------------------------------------------------------------- 1. ties
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["twins", "twins_mega", "stack"])
def test_ties(renderer, name, prec):
    """Spheres with equal t and different albedo: hit_update's tie rule (rt_sweep.hpp: fp64 select, fp32 64-bit
    key; the later scene index wins, objects.rs:141) decides `hi` and with it the albedo output.  twins: pairs far
    apart in scene and slot order (both grounds in the always-exact group); twins_mega: 2 200 spheres through the
    MEGA cone walk; stack: 40 coincident spheres over three clusters, an overflowing pixel list.  With the
    materials exchanged (swap / reverse) the geometry is unchanged, so depth, normal and coverage equal the
    first run's bit for bit and the albedo is the exchanged restatement's."""
    mega = name == "twins_mega"
    got, st = run(renderer, (name, False), prec, mega=mega)
    assert abi.kernel_info(st.kernel_id)["mega"] is mega
    other, _ = run(renderer, (name, True), prec, mega=mega)
    assert_guides_equal(other, got, names=GEOMETRY)
    assert (other["albedo"] != got["albedo"]).any()
    if name == "stack":
        assert fell_back(renderer, (name, False), prec)   # 40 slots pass together: more than a list holds


@pytest.mark.parametrize("prec", PRECS)
def test_twins_filter_off_same_guides(renderer, prec, monkeypatch):
    """With RT_FILTER_OFF=1 every cone-cull record passes (rp = +inf, build_cam_table), so every pixel list
    overflows and every batch tests every sphere: a false cull of one member of a tie would show between the two."""
    filtered, _ = run(renderer, ("twins", False), prec)
    monkeypatch.setenv("RT_FILTER_OFF", "1")
    off, _ = run(renderer, ("twins", False), prec)
    assert_guides_equal(off, filtered)


# ---------------------------------------------------------------- 2. radii
@pytest.mark.parametrize("prec", PRECS)
def test_radii(renderer, prec):
    """Radii -1, -0.9, -0.2, 0, 1e-12 and a -r / +r pair.  On the live path r enters only squared: pack_scene's
    field() stores r^2 for the exact test (objects.rs:256), build_cam_table's camera-origin record subtracts that
    r^2 and its cone record takes sqrt(r^2 ...), and guide_pixels takes the normal from (loc - c) / |loc - c| and
    the sign from d . u (rt_guides.hpp, objects.rs:158-161), never from c / r.  So ALL FOUR outputs of radii and of
    radii(absolute=True) agree bit for bit (the material indices are the same): asserted.  The pair's winner is the
    later index, the +1 Lambertian (tests/test_guide_edges.py shows the tie is in view)."""
    got, _ = run(renderer, ("radii", False), prec)
    absolute, _ = run(renderer, ("radii", True), prec)
    assert_guides_equal(absolute, got)


# ---------------------------------------------------------------- 3. materials
@pytest.mark.parametrize("prec", PRECS)
def test_materials(renderer, prec):
    """The material table's extremes: six Dielectrics give albedo 1 whatever their ior, the Metals and Lambertians
    their albedo (0 and 1 among them) rounded to T by the host's MatT precompute."""
    run(renderer, ("materials",), prec)


# ---------------------------------------------------------------- 4. scaled
@pytest.mark.parametrize("s", es.SCALES)
@pytest.mark.parametrize("prec", PRECS)
def test_scaled(renderer, prec, s):
    """random_spheres(100) and its camera scaled by s (test_gpu_scene_edges.test_scaled's docstring reads the
    culls at each scale).  Depth is t cast to float32: 1e7 .. 9e26 here, finite.  fp32 at 1e19 and 1e25: pure sky
    (|c|^2 overflows in the exact test), albedo 1 and zeros.  fp64 at 1e19 and 1e25: the cone records have
    rp = +inf (kConeWMax, rt_camera.hpp), every list overflows, every sphere reaches the exact test."""
    got, _ = run(renderer, ("scaled", s), prec)
    if prec == "f32" and s >= 1e19:
        assert not got["coverage"].any()
    else:
        assert (got["coverage"] > 0).any() and np.isfinite(got["depth"]).all()
    if prec == "f64" and s >= 1e19:
        assert fell_back(renderer, ("scaled", s), prec)


@pytest.mark.parametrize("prec", PRECS)
def test_scaled_empty(renderer, prec):
    """The 1e25 camera over no spheres: exactly albedo 1 and zeros, no sign bit set."""
    flat, cam = es.scaled(1e25, 16, 9, empty=True)
    got, st = guides(renderer, prec, 4, flat, cam)
    np.testing.assert_array_equal(got["albedo"], np.ones((144, 3), np.float32))
    for name in GEOMETRY:
        assert not got[name].any() and not np.signbit(got[name]).any(), name
    check_stats(st, 144, 4, prec, camq=True, mega=False)


# ---------------------------------------------------------------- 5. needles
@pytest.mark.parametrize("kind", es.NEEDLES)
@pytest.mark.parametrize("prec", PRECS)
def test_needle(renderer, prec, kind):
    """Rays all but parallel to an axis from a camera that is no pinhole to the launch (the -0.0 in the centre, or
    the lens): guide_pixels<T, false, false>, the primary rays through nearest_hit's general sweep, zero-basis lanes
    (L < 1e-15, rt_sweep.hpp) mixed with ordinary ones in down_1e-6, inv_ax's clamps in along_x.  Bounce 0 is the
    whole result here."""
    run(renderer, ("needle", kind), prec, camq=False)


@pytest.mark.parametrize("prec", PRECS)
def test_needle_filter_off_same_guides(renderer, prec, monkeypatch):
    filtered, _ = run(renderer, ("needle", "down_1e-6"), prec, camq=False)
    monkeypatch.setenv("RT_FILTER_OFF", "1")
    off, _ = run(renderer, ("needle", "down_1e-6"), prec, camq=False)
    assert_guides_equal(off, filtered)


# ---------------------------------------------------------------- 6. layout families
@pytest.mark.parametrize("name", sorted(es.LAYOUT_FAMILIES))
@pytest.mark.parametrize("prec", PRECS)
def test_layout_families(renderer, prec, name):
    """build_layout's shapes (test_gpu_scene_edges.test_layout_families reads them) under the guide kernel's
    lists.  count1: one sphere in one cluster of dummies, so a list holds at most slot 0 and a batch runs at most
    one exact test, listed or not.  concentric: 50 shells at one centre, more than a list holds wherever the
    cone meets them, so some pixel falls back to the per-batch sweep."""
    key = ("layout", name)
    _, st = run(renderer, key, prec)
    if name == "count1":
        assert 0 < st.camera_exact_tests <= 144   # one batch per pixel at 4 spp
        assert not fell_back(renderer, key, prec)
    if name == "concentric":
        assert fell_back(renderer, key, prec)


# ---------------------------------------------------------------- 7. defocus with MEGA
@pytest.mark.parametrize("prec", PRECS)
def test_defocus_mega(renderer, prec):
    """guide_pixels<T, false, true>: config E's 10 000 spheres through a lens, every primary ray through
    nearest_hit<T, false, false, true> (the super level of the general sweep) at bounce 0."""
    _, idx = samples(("defocus_mega",), prec)
    assert len(np.unique(idx)) > 8
    _, st = run(renderer, ("defocus_mega",), prec, camq=False, mega=True)
    k = abi.kernel_info(st.kernel_id)
    assert k["guides"] and k["mega"] and not k["camq"]
    assert abi.kernel_name(st.kernel_id) == f"guide_pixels<{'float' if prec == 'f32' else 'double'},false,true>"


# ---------------------------------------------------------------- 8. the list boundary
@pytest.mark.parametrize("prec", PRECS)
def test_list_boundary(renderer, prec):
    """stack(n=k), k = 1 .. 9, through a one-pixel range on the stack: the k coincident spheres have one and the
    same cone record, so they pass pixel_list's walk together and the list grows by one per k until it holds
    kCList - 1 = 7 slots (rt_camera.hpp); one more and list[0] = 0xFFFF, the pixel's batches run camera_sweep.
    Whether the ground (always exact, slot 0) is in the pixel's cone too is not assumed: the flip is found from
    the statistics.  A full list is the edge of fp64's camera_listed, which unpacks the 8 u16 entries from four
    SGPR words and prefetches entry(j + 2).  Every k is compared at 1, 64 and 65 spp (one lane, a full batch,
    a second batch with one lane)."""
    listed, length = {}, {}
    for k in range(1, 10):
        key = ("stackn", k)
        st = {spp: run(renderer, key, prec, spp=spp)[1] for spp in (1, 64, 65)}
        assert st[65].cone_tests >= st[1].cone_tests > 0, k
        listed[k] = st[65].cone_tests == st[1].cone_tests
        if listed[k]:
            length[k] = st[64].camera_exact_tests
            # one exact test per listed slot and batch
            assert (st[1].camera_exact_tests, st[65].camera_exact_tests) == (length[k], 2 * length[k]), k
            assert st[64].cone_tests == st[1].cone_tests
        else:
            # the sweep tests every passing slot once per batch: at least the k members, which the restatement hits
            assert st[64].camera_exact_tests >= k and st[65].camera_exact_tests == 2 * st[64].camera_exact_tests, k
    ks = sorted(length)
    assert ks and ks == list(range(1, ks[-1] + 1)), listed          # listed up to some k, fallback from there on
    assert 1 <= length[1] <= 2                                         # the one sphere, with or without the ground
    assert [length[k] - length[1] for k in ks] == [k - 1 for k in ks]   # one more slot per coincident sphere
    full = ks[-1]
    assert length[full] == 7, length                                   # a full list: kCList - 1 entries
    assert full + 1 <= 9 and not listed[full + 1], listed             # and the next k falls back


# ---------------------------------------------------------------- 9. spp at its limit
@pytest.mark.parametrize("prec", PRECS)
def test_spp_limit_on_one_pixel(renderer, prec):
    """spp = 1 << 20, the most rt_render_guides_async takes, on one pixel whose whole footprint lies on one
    Lambertian sphere seen from outside (tests/test_guide_edges.py: every restated ray hits): 16 384 batches of one
    wave, sample ids up to 2^20 - 1 in the fp32 counter's 20 bits.  Every sample hits, so coverage is exactly 1 and
    each albedo channel is the definition's fold of 2^20 equal values a (the material's albedo in T).  Normal and
    depth are not restated at this count: finite, the normal inside the unit ball, the depth between the sphere's
    nearest point and its tangent distance from the camera, which contain the 256 restated samples' range."""
    key = ("cover",)
    flat, cam, _, _ = case(key)
    run(renderer, key, prec, spp=256)
    n = 1 << 20
    got, st = guides(renderer, prec, n, flat, cam, tile=tile_of(key))
    check_stats(st, 1, n, prec, camq=True, mega=False)
    assert st.samples == st.ray_segments == n
    assert got["coverage"].tolist() == [1.0]
    albedo = iv.scene_from_flat(flat, prec)[2][0].albedo   # rounded as the kernel's material table is
    want = [fold(np.full(n, float(a))) for a in albedo]
    np.testing.assert_array_equal(got["albedo"], np.array([want], dtype=np.float32))
    assert np.isfinite(got["normal"]).all() and np.isfinite(got["depth"]).all()
    vals, _ = samples(key, prec)
    near, far = cover_geometry()
    assert near <= vals[:, :, 6].min() and vals[:, :, 6].max() <= far
    assert np.float32(near) <= got["depth"][0] <= np.float32(far)
    assert 0.0 < math.sqrt(float((got["normal"].astype(np.float64) ** 2).sum())) <= 1.0


# ---------------------------------------------------------------- 10. wide cone
@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("prec", PRECS)
def test_wide_cone(renderer, prec, w):
    """A w x 1 frame at a view angle of 150 degrees: the footprint's corners are more than 60 degrees off its
    axis, so pixel_list reports `over` before any walk (dt <= 0.5, S >= 0.5; rt_camera.hpp) and both batches of
    65 spp run camera_sweep, whose own cone is as wide (`all`: every record to the exact test)."""
    key = ("wide", w)
    run(renderer, key, prec)
    assert fell_back(renderer, key, prec)


# ---------------------------------------------------------------- 11. slots past u16
@pytest.mark.parametrize("prec", PRECS)
def test_slots_past_u16(renderer, prec):
    """70 000 spheres: slot indices past 0xFFFF, which a u16 list entry cannot hold (sl >= 0xFFFF: over,
    rt_camera.hpp), under the MEGA cone walk; 4 x 3 x 2 spp, test_mega_walk_shapes' shape."""
    key = ("slots",)
    flat = case(key)[0]
    _, idx = samples(key, prec)
    hit = idx[idx >= 0]
    assert (np.abs(flat.radius[hit]) < 1.0).any()
    _, st = run(renderer, key, prec, mega=True)
    assert abi.kernel_info(st.kernel_id)["mega"]
    assert fell_back(renderer, key, prec)
