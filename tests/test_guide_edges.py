"""The scenes of tests/test_gpu_guide_edges.py do, on the restatement alone (tests/guide_restatement.py), what the
GPU tests need them for: a guide test on twins that never tie in view, on negative spheres out of frame or on a
scaled scene that is all sky would pass without reaching the branch it is named for.  What tests/test_edge_scenes.py
does on the oracle for the render kernels, this file does on the restatement for guide_pixels.

Every assertion is a condition on the INPUT (the scene, the camera, the samples), none a measurement of the
kernel.  case() is the one table of frames and sample counts; the GPU tests take their scenes from it, so both
files speak of the same samples.  The last part checks the restatement itself: independent_v2's candidate
estimate against the literal test of every sphere, on every sample the GPU tests use.
"""
import math

import numpy as np
import pytest

import edge_scenes as es
import independent_v2 as iv
import rt_mi355x as rt
from rt_mi355x import abi
from guide_restatement import SEED, cam_dict, restate_guides, restate_samples, samples_once

PRECS = ("f64", "f32")
F32_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------- the cases: (flat, cam, spp, pixels)
def cam_for(w, h, **kw):
    return rt.camera_new_py(w, h, **dict(rt.MAIN_CAMERA, **kw))


_built = {}


def _once(key, build):
    if key not in _built:
        _built[key] = build()
    return _built[key]


def scene_100():
    return _once("s100", lambda: rt.scenes.random_spheres(100).flatten())


def stack_pixel():
    """The pixel of the 16x9 stack frame that case 8 traces alone: of the pixels whose 8 restated samples
    all hit the stack (not the ground), the one nearest the frame's centre."""
    def pick():
        _, idx = samples(("stack", False), "f64")
        full = np.flatnonzero((idx >= 1).all(axis=1))
        assert len(full) > 0
        d2 = (full // 16 - 4.0) ** 2 + (full % 16 - 7.5) ** 2
        return int(full[np.argmin(d2)])
    return _once("stack_pixel", pick)


def case(key):
    """(flat, cam, spp, pixels) of a case of tests/test_gpu_guide_edges.py; spp is the largest count it is run at
    and pixels None (the whole frame) or the one pixel of its tile range.  Built once per key."""
    def build():
        kind = key[0]
        if kind == "twins":
            return es.twins(100, 16, 9, swap=key[1]) + (12, None)
        if kind == "twins_mega":
            return es.twins_mega(swap=key[1]) + (16, None)
        if kind == "stack":
            return es.stack(16, 9, reverse=key[1]) + (8, None)
        if kind == "radii":
            return es.radii(16, 9, absolute=key[1]) + (8, None)
        if kind == "materials":
            return es.materials(16, 9) + (6, None)
        if kind == "scaled":
            return es.scaled(key[1], 16, 9) + (4, None)
        if kind == "needle":
            return es.needle(key[1]) + (6, None)
        if kind == "layout":
            return es.LAYOUT_FAMILIES[key[1]]() + (4, None)
        if kind == "defocus_mega":
            flat = _once("E", lambda: rt.scenes.config_scene("E").flatten())
            return flat, cam_for(16, 9, defocus_angle=0.6), 6, None
        if kind == "stackn":
            return es.stack(16, 9, n=key[1]) + (65, [stack_pixel()])
        if kind == "cover":
            return es.cover(3, 3) + (256, [4])
        if kind == "wide":
            return scene_100(), cam_for(key[1], 1, view_angle=150.0), 65, None
        if kind == "slots":
            return _once("s70000", lambda: rt.scenes.random_spheres(70000).flatten()), cam_for(4, 3), 2, None
        raise KeyError(key)
    return _once(("case", key), build)


def samples(key, prec):
    """restate_samples of case(key) at its largest count: (vals [P, spp, 8], idx [P, spp]), once per (key, prec)."""
    flat, cam, spp, pixels = case(key)
    return samples_once(("edges",) + key + (prec,), flat, cam, spp, prec, pixels=pixels)   # no key of test_gpu_guides


def tile_of(key):
    """The RtTileRange of a one-pixel case (None: the whole frame)."""
    _, cam, _, pixels = case(key)
    if pixels is None:
        return None
    (pix,) = pixels
    return abi.RtTileRange(row_begin=pix // cam.image_width, row_step=1, row_count=1, col_begin=pix % cam.image_width,
                           col_count=1)


def rays(key, prec):
    """(pixel index, sample, origin, direction) of every sample of a case, as restate_samples walks them."""
    flat, cam, spp, pixels = case(key)
    camp = iv.camera_in(cam_dict(cam), prec)
    W = cam.image_width
    for k, pix in enumerate(range(W * cam.image_height) if pixels is None else pixels):
        for s in range(spp):
            yield (k, s) + iv.get_ray(camp, pix % W, pix // W, s, pix, SEED, prec)


def literal_scene(key, prec):
    return _once(("literal", key, prec), lambda: iv.scene_from_flat(case(key)[0], prec, literal=True)[0])


def valid_roots(spheres, o, d):
    """The literal test of EVERY sphere for one ray (iv.hit_scene's loop body, objects.rs:252-277, without the
    update): {scene index: root1} of the spheres whose root is valid."""
    out = {}
    a = iv.pk_len2(d)
    inv_a = 1.0 / a
    for i, (c, r2) in enumerate(spheres):
        oc = iv.v_sub(o, c)
        hb = iv.pk_dot(oc, d)
        disc = iv.fma(hb, hb, (-a) * (iv.pk_len2(oc) - r2))
        if not disc >= 0.0:
            continue
        root = (-hb - iv.sqrt(disc)) * inv_a
        if root >= 0.001 and root < math.inf:
            out[i] = root
    return out


def albedo_of(flat, i):
    m = flat.materials[int(flat.material[i])].to_abi()
    return (1.0, 1.0, 1.0) if m.kind == abi.RT_DIELECTRIC else tuple(m.albedo)


# ---------------------------------------------------------------- ties
def tied_samples(key, prec):
    """Over the hit samples of a case: how many have a winning t that a second sphere of another albedo shares,
    from the literal test of every sphere."""
    flat = case(key)[0]
    vals, idx = samples(key, prec)
    lit = literal_scene(key, prec)
    n = 0
    for k, s, o, d in rays(key, prec):
        if idx[k, s] < 0:
            continue
        roots = valid_roots(lit, o, d)
        w = int(idx[k, s])
        assert float(roots[w]) == vals[k, s, 6] and roots[w] == min(roots.values())
        n += any(i != w and t == roots[w] and albedo_of(flat, i) != albedo_of(flat, w) for i, t in roots.items())
    return n


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["twins", "twins_mega", "stack"])
def test_ties_decide_the_albedo(name, prec):
    """The nearest hit is shared by spheres of different albedo on most hit samples (every sphere of twins has a
    twin, every stack hit 40 members), so a wrong winner is a wrong number in `albedo`.  Exchanging the
    materials (swap / reverse) leaves the geometry alone: the per-sample depth, normal and coverage are the same
    arrays, and the albedo output changes on every pixel with a tied hit whose albedo sum moves."""
    key, other = (name, False), (name, True)
    assert tied_samples(key, prec) > 0
    va, ia = samples(key, prec)
    vb, ib = samples(other, prec)
    np.testing.assert_array_equal(va[:, :, 3:], vb[:, :, 3:])
    np.testing.assert_array_equal(ia, ib)
    spp = case(key)[2]
    ga, gb = restate_guides(va, spp), restate_guides(vb, spp)
    for out in ("normal", "depth", "coverage"):
        np.testing.assert_array_equal(ga[out], gb[out])
    hit = ga["coverage"] > 0
    moved = (ga["albedo"] != gb["albedo"]).any(axis=1)
    assert hit.any() and not moved[~hit].any()
    if name == "stack":
        # the winner is the last of the 40 (objects.rs:141, t <= best) wherever the stack is hit, and the ground
        # (index 0, untied) wherever it is not
        assert set(np.unique(ia).tolist()) == {-1, 0, 40}
        on_stack = (ia == 40).any(axis=1)
        assert on_stack.any() and moved[on_stack].all() and not moved[~on_stack].any()
    else:
        assert moved[hit].all()   # the ground is twinned too: every hit is a tie


# ---------------------------------------------------------------- signed radii
@pytest.mark.parametrize("prec", PRECS)
def test_radii_reach_the_negative_spheres(prec):
    """es.radii's spheres by scene index: 0 ground, 1 glass (r 1) around 2 (r -0.9, the bubble), 3 (r -1), 4
    (r 0), 5 (r 1e-12), 6 (r -0.2), 7 / 8 the -1 / +1 pair at one centre.

    Spheres 3 and 6 are some sample's nearest hit.  The bubble never is: its literal test gives a valid root on
    some samples (the exact test and hit_update run for it), always behind the shell's.  Of the pair, 8 (+1, the
    later index) wins every tie with 7 (objects.rs:141); 7 has the same t on exactly those samples.

    `front` (objects.rs:160) is true on every hit: hit_packed takes root1 alone (quirk Q1), the near root of a ray
    that starts outside, where the unit normal faces the ray; r enters only as r.powi(2), so a negative radius
    does not turn it.  front false at bounce 0 needs a ray whose near root is at a tangent within rounding; this
    scene has none in either precision, so `nrm = neg(u)` (rt_guides.hpp) is not reached by it."""
    key = ("radii", False)
    vals, idx = samples(key, prec)
    winners = set(np.unique(idx).tolist())
    assert {3, 6, 8} <= winners and 2 not in winners and 7 not in winners
    lit = literal_scene(key, prec)
    spheres = iv.scene_from_flat(case(key)[0], prec)[0]
    bubble = pair = 0
    fronts = set()
    for k, s, o, d in rays(key, prec):
        if idx[k, s] < 0:
            continue
        roots = valid_roots(lit, o, d)
        fronts.add(bool(iv.hit_scene(spheres, o, d)[3]))
        if 2 in roots:
            bubble += 1
            assert roots[1] < roots[2]
        assert (7 in roots) == (8 in roots)
        if idx[k, s] == 8:
            pair += 1
            assert roots[7] == roots[8]
    assert bubble > 0 and pair > 0
    assert fronts == {True}
    # |r| for r: the same samples, bit for bit (r only squared)
    va, ia = samples(("radii", True), prec)
    np.testing.assert_array_equal(va, vals)
    np.testing.assert_array_equal(ia, idx)


# ---------------------------------------------------------------- materials
@pytest.mark.parametrize("prec", PRECS)
def test_materials_all_hit(prec):
    """Every one of es.materials' 12 spheres is some sample's first hit, and every Dielectric sample has albedo 1."""
    flat = case(("materials",))[0]
    vals, idx = samples(("materials",), prec)
    assert set(range(12)) <= set(np.unique(idx).tolist())
    kinds = np.array([flat.materials[int(m)].to_abi().kind for m in flat.material])
    glass = (idx >= 0) & (kinds[np.maximum(idx, 0)] == abi.RT_DIELECTRIC)
    assert glass.any() and (vals[glass][:, 0:3] == 1.0).all()
    assert (kinds == abi.RT_DIELECTRIC).sum() == 6
    other = (idx >= 0) & ~glass
    assert (vals[other][:, 0:3] != 1.0).any()


# ---------------------------------------------------------------- scaled
@pytest.mark.parametrize("s", es.SCALES)
@pytest.mark.parametrize("prec", PRECS)
def test_scaled_hits_and_sky(prec, s):
    """Hits and sky both occur at every scale in fp64, and up to 1e16 in fp32.  At 1e19 and 1e25 the fp32
    restatement gives pure sky, as the oracle does (test_gpu_scene_edges.test_scaled's docstring): |c|^2
    overflows in the exact test.  Depth is t itself cast to float32: finite in float32 on every pixel that has
    coverage (the largest t is about 90 s; at 1e25 that is 9e26)."""
    vals, idx = samples(("scaled", s), prec)
    g = restate_guides(vals, 4)
    if prec == "f32" and s >= 1e19:
        assert (idx < 0).all()
        np.testing.assert_array_equal(g["coverage"], np.zeros(144, np.float32))
        np.testing.assert_array_equal(g["albedo"], np.ones((144, 3), np.float32))
        return
    assert (g["coverage"] > 0).any() and (g["coverage"] == 0).any()
    assert np.isfinite(g["depth"][g["coverage"] > 0]).all() and (g["depth"][g["coverage"] > 0] > 0).all()
    assert vals[:, :, 6].max() > 10.0 * s and vals[:, :, 6].max() < F32_MAX
    for name in ("albedo", "normal", "depth", "coverage"):
        assert np.isfinite(g[name]).all(), name


@pytest.mark.parametrize("prec", PRECS)
def test_scaled_empty_is_sky(prec):
    flat, cam = es.scaled(1e25, 16, 9, empty=True)
    vals, idx = restate_samples(flat, cam, 4, prec)
    assert (idx < 0).all() and (vals[:, :, 0:3] == 1.0).all() and not vals[:, :, 3:].any()


# ---------------------------------------------------------------- needles
@pytest.mark.parametrize("kind", es.NEEDLES)
@pytest.mark.parametrize("prec", PRECS)
def test_needles_hit(prec, kind):
    """Every one of a needle's 48 x 3 x 6 primary rays hits the same sphere, never the sky: the strip spans 1.4e-7
    rad, a width of 4e-6 at the sphere, so hits and misses cannot both occur in one frame (the down cameras sit
    over the glass sphere at (0, 1, 0), t = 28; along_x meets a small one at t = 15.4).  A wrong cull of that
    sphere on any lane is then a coverage below 1, a depth and a normal off the restated ones: the guides the
    GPU test compares are no constants of an empty frame."""
    vals, idx = samples(("needle", kind), prec)
    assert (idx >= 1).all() and len(np.unique(idx)) == 1, kind
    assert (vals[:, :, 6] > 15.0).all() and (vals[:, :, 6] < 28.5).all()
    g = restate_guides(vals, 6)
    assert (g["coverage"] == 1).all() and (g["depth"] > 15).all() and (np.abs(g["normal"]).max(axis=1) > 0.5).all()


# ---------------------------------------------------------------- the single-pixel and kernel-path cases
@pytest.mark.parametrize("prec", PRECS)
def test_stack_pixel_is_covered_for_every_k(prec):
    """Case 8's pixel: all 65 samples hit the stack, whose last member (index k) wins, for k = 1 .. 9."""
    for k in range(1, 10):
        vals, idx = samples(("stackn", k), prec)
        assert (idx == k).all(), k
        assert (vals[:, :, 7] == 1.0).all()


def cover_geometry():
    """(near, far): the distances from the camera to the covering sphere's nearest point and to its tangent
    points, the range of every first-hit t on it."""
    _, cam, _, _ = case(("cover",))
    dist = math.dist(tuple(cam.center), es.COVER_CENTER)
    assert dist > es.COVER_RADIUS   # the camera is outside (quirk Q1)
    return dist - es.COVER_RADIUS, math.sqrt(dist * dist - es.COVER_RADIUS ** 2)


@pytest.mark.parametrize("prec", PRECS)
def test_cover_is_hit_by_every_ray(prec):
    """Case 9's pixel: 256 of 256 restated rays hit the one sphere, at depths inside the geometric range; the
    footprint's corners are further inside the sphere's silhouette than any of them."""
    flat, cam, _, _ = case(("cover",))
    assert flat.n_spheres == 1
    vals, idx = samples(("cover",), prec)
    assert (idx == 0).all()
    near, far = cover_geometry()
    assert near <= vals[:, :, 6].min() and vals[:, :, 6].max() <= far
    # the whole 3 x 3 frame lies inside the silhouette: its farthest corner's angle from the axis is below the
    # sphere's angular radius
    axis = np.array(es.COVER_CENTER) - np.array(cam.center)
    half = math.asin(es.COVER_RADIUS / np.linalg.norm(axis))
    ulc, vu, vv = np.array(cam.ulc), np.array(cam.vu), np.array(cam.vv)
    for fx in (0.0, 1.0):
        for fy in (0.0, 1.0):
            dd = ulc + fx * vu + fy * vv - np.array(cam.center)
            ang = math.acos(dd @ axis / np.linalg.norm(dd) / np.linalg.norm(axis))
            assert ang < 0.9 * half


@pytest.mark.parametrize("prec", PRECS)
def test_defocus_mega_sees_many_spheres(prec):
    _, idx = samples(("defocus_mega",), prec)
    assert len(np.unique(idx)) > 8 and (idx < 0).any()
    assert case(("defocus_mega",))[0].n_spheres == 10000


@pytest.mark.parametrize("w", [1, 2])
def test_wide_cone_corners_are_past_60_degrees(w):
    """Case 10: every pixel's footprint has a corner more than 60 degrees off the pixel's axis (pixel_list's `over`
    before any walk: some corner's cosine is not above 0.5, rt_camera.hpp), and the rays both hit and miss."""
    _, cam, _, _ = case(("wide", w))
    ulc, vu, vv, cen = (np.array(x) for x in (cam.ulc, cam.vu, cam.vv, cam.center))
    for col in range(w):
        axis = ulc + vu * (col + 0.5) / w + vv * 0.5 - cen
        cos = []
        for fx in (0.0, 1.0):
            for fy in (0.0, 1.0):
                dd = ulc + vu * (col + fx) / w + vv * fy - cen
                cos.append(dd @ axis / np.linalg.norm(dd) / np.linalg.norm(axis))
        assert min(cos) < 0.49, (col, cos)
    for prec in PRECS:
        _, idx = samples(("wide", w), prec)
        assert (idx >= 0).any() and (idx < 0).any()


@pytest.mark.parametrize("prec", PRECS)
def test_slots_scene_hits_a_small_sphere(prec):
    """Case 11: 70 000 spheres (more slots than a u16 index holds), and some sample's first hit is a small one."""
    flat = case(("slots",))[0]
    assert flat.n_spheres == 70000 > 0xFFFF
    _, idx = samples(("slots",), prec)
    hit = idx[idx >= 0]
    assert (np.abs(flat.radius[hit]) < 1.0).any()


# ---------------------------------------------------------------- the restatement's own estimate
SELF_CHECK = ([("twins", False), ("twins_mega", False), ("stack", False), ("radii", False), ("materials",)]
              + [("scaled", s) for s in es.SCALES] + [("needle", kind) for kind in es.NEEDLES]
              + [("stackn", 9), ("cover",), ("wide", 2)])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", SELF_CHECK, ids=lambda k: "-".join(str(x) for x in k))
def test_estimate_drops_nothing(key, prec):
    """hit_scene with independent_v2's candidate estimate (tolerance 1e-9 / 1e-4 relative to hb^2 + a (|oc|^2 +
    r^2), written for ordinary scales) returns the same (t, index) as with every sphere tested, on every sample
    the GPU tests use: the estimate is scale-free (both sides scale alike) and keeps NaN and inf, so it drops
    nothing at 1e25, on the needles or on the ties.  The swapped / reversed / absolute variants share the
    geometry of the scenes listed, and the 10 000- and 70 000-sphere scenes are ordinary in scale."""
    flat = case(key)[0]
    est = iv.scene_from_flat(flat, prec)[0]
    lit = literal_scene(key, prec)
    vals, idx = samples(key, prec)
    for k, s, o, d in rays(key, prec):
        a, b = iv.hit_scene(est, o, d), iv.hit_scene(lit, o, d)
        assert (a is None) == (b is None), (k, s)
        if a is not None:
            assert (a[0], a[4]) == (b[0], b[4]), (k, s)
            assert (float(a[0]), a[4]) == (vals[k, s, 6], idx[k, s])
        else:
            assert idx[k, s] == -1
