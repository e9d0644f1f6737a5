"""Degenerate scenes shared by tests/test_edge_scenes.py (CPU: each scene does on the oracle what it is
meant to) and tests/test_gpu_scene_edges.py (GPU: the HIP kernels against the oracle on them), and by
tests/test_guide_edges.py and tests/test_gpu_guide_edges.py (the guide kernel against its restatement on them).

Plain module: no GPU, no fixtures.  Every builder is deterministic (fixed numpy seeds) and returns
(FlatScene, RtCamera).  The cameras of the scenes the independent restatement also renders are module
constants (its camera_new takes the same keywords).  Frames stay at or below 48x27.
"""
import numpy as np

import rt_mi355x as rt

SEED = 0x5EED0001


def camera(w, h, **kw):
    return rt.camera_new_py(w, h, **dict(rt.MAIN_CAMERA, **kw))


# ---------------------------------------------------------------- ties
def _other_material(m):
    """A visibly different material of another kind."""
    if isinstance(m, rt.Lambertian):
        return rt.Metal((0.95, 0.35, 0.3), 0.25)
    if isinstance(m, rt.Metal):
        return rt.Dielectric(1.5, False)
    return rt.Lambertian((0.15, 0.3, 0.85))


TWINS_CAMERA = dict(rt.MAIN_CAMERA)


def twins(n=100, w=16, h=9, swap=False):
    """random_spheres(n) twice: copy k sits at index 2n-1-k with another material, so the members of a pair are
    far apart in scene order (and in slot order: one ground in the always-exact group at slot 0, its twin at
    slot 1; the 2 x 3 big spheres there too; the small ones in clusters with their twins).
    swap: the two members of every pair exchange materials (the geometry is unchanged)."""
    base = rt.scenes.random_spheres(n).flatten()
    mats = list(base.materials) + [_other_material(m) for m in base.materials]
    first = base.material.astype(np.uint32)
    second = (base.material[::-1] + len(base.materials)).astype(np.uint32)
    if swap:
        first, second = first + len(base.materials), second - len(base.materials)
    flat = rt.FlatScene(np.concatenate([base.center, base.center[::-1]]),
                        np.concatenate([base.radius, base.radius[::-1]]),
                        np.concatenate([first, second]), mats)
    return flat, camera(w, h, **TWINS_CAMERA)


def twins_mega(w=8, h=5, swap=False):
    """twins from random_spheres(1100): 2 200 spheres, 2 192 of them filtered, more than 8 super groups, so the
    mega kernels walk them in group-local and cluster-local frames."""
    return twins(1100, w, h, swap)


STACK_CAMERA = dict(rt.MAIN_CAMERA, center=(2.5, 1.5, 3.0), look_at=(0.0, 1.0, 0.0))


def stack(w=16, h=9, reverse=False, n=40):
    """Ground plus n (40) identical spheres (centre (0, 1, 0), radius 1) with n distinct Lambertian albedos; the
    camera is 4 units away.  reverse: the n materials in the opposite order."""
    rng = np.random.default_rng(41)
    albedo = rng.uniform(0.05, 0.95, (n, 3))
    mats = [rt.Lambertian((0.5, 0.5, 0.5))] + [rt.Lambertian(tuple(a)) for a in albedo]
    order = np.arange(1, n + 1)
    if reverse:
        order = order[::-1]
    center = np.array([[0.0, -1000.0, 0.0]] + [[0.0, 1.0, 0.0]] * n)
    radius = np.array([1000.0] + [1.0] * n)
    flat = rt.FlatScene(center, radius, np.concatenate([[0], order]).astype(np.uint32), mats)
    return flat, camera(w, h, **STACK_CAMERA)


COVER_ALBEDO = (0.3, 0.55, 0.7)
COVER_CENTER, COVER_RADIUS = (0.0, 1.0, 0.0), 2.0


def cover(w=3, h=3):
    """One Lambertian sphere (radius 2 at (0, 1, 0)) and no ground under the stack's camera, which looks at its
    centre from outside: the middle pixel of a small odd frame has its whole footprint on the sphere."""
    flat = rt.FlatScene(np.array([COVER_CENTER]), np.array([COVER_RADIUS]), np.zeros(1, np.uint32),
                        [rt.Lambertian(COVER_ALBEDO)])
    return flat, camera(w, h, **STACK_CAMERA)


# ---------------------------------------------------------------- signed and zero radii
RADII_CAMERA = dict(rt.MAIN_CAMERA, center=(0.0, 1.4, 6.5), look_at=(0.0, 0.8, 0.0), view_angle=36.0)


def radii(w=16, h=9, absolute=False):
    """Ground; a glass sphere with a -0.9 bubble inside it; spheres of radius -1, 0, 1e-12 and -0.2; a -r / +r
    pair at one centre with different materials (the negative one first: scalar mode's tie rule shows it).
    absolute: every radius replaced by its absolute value."""
    glass = rt.Dielectric(1.5, False)
    objs = [
        ((0.0, -1000.0, 0.0), 1000.0, rt.Lambertian((0.5, 0.5, 0.5))),
        ((-2.3, 1.0, 0.0), 1.0, glass),
        ((-2.3, 1.0, 0.0), -0.9, glass),
        ((0.0, 1.0, 0.0), -1.0, rt.Lambertian((0.8, 0.3, 0.2))),
        ((-1.1, 0.4, 1.6), 0.0, rt.Lambertian((0.2, 0.8, 0.2))),
        ((-0.6, 0.4, 1.6), 1e-12, rt.Metal((0.9, 0.9, 0.2), 0.0)),
        ((1.15, 0.2, 1.6), -0.2, rt.Metal((0.8, 0.8, 0.9), 0.1)),
        ((2.3, 1.0, 0.0), -1.0, rt.Metal((0.9, 0.7, 0.5), 0.05)),
        ((2.3, 1.0, 0.0), 1.0, rt.Lambertian((0.2, 0.3, 0.8))),
    ]
    r = np.array([o[1] for o in objs])
    if absolute:
        r = np.abs(r)
    flat = rt.FlatScene(np.array([o[0] for o in objs]), r, np.arange(len(objs), dtype=np.uint32), [o[2] for o in objs])
    return flat, camera(w, h, **RADII_CAMERA)


# ---------------------------------------------------------------- material extremes
MATERIALS_CAMERA = dict(rt.MAIN_CAMERA, center=(0.0, 2.2, 7.5), look_at=(0.0, 0.5, 0.0), view_angle=40.0)


def materials(w=16, h=9):
    """One sphere each of the material table's extremes, in two rows on a ground."""
    mats = [rt.Dielectric(1.5, True), rt.Dielectric(2.4, True), rt.Metal((0.8, 0.8, 0.8), 1.0),
            rt.Metal((0.8, 0.6, 0.4), -0.5), rt.Metal((1.0, 1.0, 1.0), 0.0), rt.Dielectric(1.0, False),
            rt.Dielectric(0.7, False), rt.Dielectric(1e-3, False), rt.Dielectric(1e3, False),
            rt.Lambertian((0.0, 0.0, 0.0)), rt.Lambertian((1.0, 1.0, 1.0))]
    assert mats[2].fuzzy_factor == 1.0 and mats[3].fuzzy_factor == -0.5   # Metal clamps only above
    center = [[0.0, -1000.0, 0.0]]
    for k in range(11):
        row, col = (0, k) if k < 6 else (1, k - 6)
        center.append([1.25 * (col - (2.5 if row == 0 else 2.0)), 0.55, -0.6 + 1.5 * row])
    flat = rt.FlatScene(np.array(center), np.array([1000.0] + [0.55] * 11), np.arange(12, dtype=np.uint32),
                        [rt.Lambertian((0.5, 0.5, 0.5))] + mats)
    return flat, camera(w, h, **MATERIALS_CAMERA)


# ---------------------------------------------------------------- numeric range
SCALES = [1e6, 1e12, 1e14, 1e16, 1e19, 1e25]


def scaled(s, w=24, h=14, empty=False):
    """random_spheres(100) and the camera scaled by s about the origin (as test_filter_scene_scales does).
    empty: the same camera over no spheres."""
    base = rt.scenes.random_spheres(100).flatten()
    if empty:
        flat = rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32), [rt.Lambertian((0.5, 0.5, 0.5))])
    else:
        flat = rt.FlatScene(base.center * s, base.radius * s, base.material, base.materials)
    kw = dict(rt.MAIN_CAMERA)
    kw["center"] = tuple(np.array(kw["center"]) * s)
    kw["look_at"] = tuple(np.array(kw["look_at"]) * s)
    kw["focal_length"] = kw["focal_length"] * s
    return flat, rt.camera_new_py(w, h, **kw)


# ---------------------------------------------------------------- degenerate lanes
NEEDLES = ["down_1e-6", "down_1e-30", "down_defocus", "along_x"]


def needle(kind, w=48, h=3):
    """random_spheres(100) under a camera whose rays are all but parallel to an axis.  The -0.0 in the centre
    keeps every variant off the pinhole shortcut, so the primary rays go through the general sweep.  The frame
    is a 48 x 3 strip: at a view angle of 1e-6 degrees (the frame's height) its rows span 1.4e-7 rad either way
    of the y axis, so the unit directions' fx^2 + fz^2 runs from ~1e-18 to 2e-14, across the 1e-15 threshold.
      down_1e-6 / down_1e-30: at (-0.0, 30, 0) looking at the origin with up = (0, 0, -1), view angle in degrees;
      down_defocus: down_1e-6 with defocus_angle 1e-7;
      along_x: at (-20, 0.2, -0.0) looking along +x through the small spheres, view angle 1e-30."""
    flat = rt.scenes.random_spheres(100).flatten()
    down = dict(rt.MAIN_CAMERA, center=(-0.0, 30.0, 0.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0))
    if kind == "down_1e-6":
        kw = dict(down, view_angle=1e-6)
    elif kind == "down_1e-30":
        kw = dict(down, view_angle=1e-30)
    elif kind == "down_defocus":
        kw = dict(down, view_angle=1e-6, defocus_angle=1e-7)
    elif kind == "along_x":
        kw = dict(rt.MAIN_CAMERA, center=(-20.0, 0.2, -0.0), look_at=(0.0, 0.2, -0.0), view_angle=1e-30)
    else:
        raise KeyError(kind)
    return flat, rt.camera_new_py(w, h, **kw)


# ---------------------------------------------------------------- layout statistics
def _mixed(rng, n):
    """n materials: Lambertian, metal and glass mixed."""
    out = []
    for _ in range(n):
        c = rng.random()
        if c < 0.6:
            out.append(rt.Lambertian(tuple(rng.uniform(0.1, 0.9, 3))))
        elif c < 0.85:
            out.append(rt.Metal(tuple(rng.uniform(0.5, 1.0, 3)), 0.3 * rng.random()))
        else:
            out.append(rt.Dielectric(1.5, False))
    return out


def _scene(center, radius, mats):
    n = len(radius)
    return rt.FlatScene(np.array(center, dtype=np.float64).reshape(-1, 3), np.array(radius, dtype=np.float64),
                        np.arange(n, dtype=np.uint32), mats)


def concentric(w=16, h=9):
    """50 shells at one centre, radii 0.05 .. 2.5: every k-d node has zero extent on every axis."""
    rng = np.random.default_rng(50)
    r = 0.05 * (1 + rng.permutation(50))
    return _scene([[0.0, 1.0, 0.0]] * 50, r, _mixed(rng, 50)), camera(w, h, center=(5.0, 2.0, 8.0), look_at=(0.0, 1.0, 0.0))


def collinear(w=16, h=9):
    """70 spheres on the x axis (the y and z extents of every k-d node are zero)."""
    rng = np.random.default_rng(70)
    x = 0.5 * (rng.permutation(70) - 34.5)
    c = np.stack([x, np.zeros(70), np.zeros(70)], axis=1)
    return _scene(c, np.full(70, 0.24), _mixed(rng, 70)), camera(w, h, center=(3.0, 2.0, 9.0), look_at=(0.0, 0.0, 0.0))


def coplanar(w=16, h=9):
    """A 20 x 15 grid in the plane z = 0 (zero z extent; equal x within a column, equal y within a row)."""
    rng = np.random.default_rng(300)
    k = rng.permutation(300)
    c = np.stack([(k % 20) - 9.5, (k // 20) - 7.0, np.zeros(300)], axis=1)
    return _scene(c, np.full(300, 0.4), _mixed(rng, 300)), camera(w, h, center=(4.0, 3.0, 30.0), look_at=(0.0, 0.0, 0.0))


def big(nb, w=16, h=9):
    """60 small spheres (radius 0.2) plus nb of 5x the radius and no ground: nb <= kBigExact = 8 big spheres
    join the always-exact group (and are the only ones in it), 9 stay in the clusters."""
    rng = np.random.default_rng(60 + nb)
    c, r = [], []
    for k in range(60):
        c.append([(k % 10) - 4.5 + 0.5 * rng.random(), 0.2, (k // 10) - 1.0 + 0.5 * rng.random()])
        r.append(0.2)
    for k in range(nb):
        c.append([2.2 * (k - (nb - 1) / 2.0), 1.0, -3.0])
        r.append(1.0)
    order = rng.permutation(60 + nb)
    return (_scene(np.array(c)[order], np.array(r)[order], _mixed(rng, 60 + nb)),
            camera(w, h, center=(0.0, 3.0, 14.0), look_at=(0.0, 0.5, 0.0), view_angle=40.0))


def uniform(w=16, h=9):
    """40 equal spheres, none far out: no always-exact sphere at all (n_xs == 0, n_xg == 0)."""
    rng = np.random.default_rng(40)
    c = rng.uniform(-3.0, 3.0, (40, 3)) * np.array([1.0, 0.5, 1.0])
    return _scene(c, np.full(40, 0.5), _mixed(rng, 40)), camera(w, h, center=(0.0, 1.0, 12.0), look_at=(0.0, 0.0, 0.0))


COUNTS = [1, 2, 5, 15, 16, 17, 33, 64, 65]


def count(n, w=16, h=9):
    """n random spheres around the cluster size (16) and the super unit (64); the first is always in view."""
    rng = np.random.default_rng(1000 + n)
    c = rng.uniform(-3.0, 3.0, (n, 3)) * np.array([1.0, 0.4, 1.0]) + np.array([0.0, 1.0, 0.0])
    r = rng.uniform(0.2, 0.6, n)
    c[0], r[0] = (0.0, 1.0, 0.0), 1.0
    return _scene(c, r, _mixed(rng, n)), camera(w, h, center=(0.0, 1.5, 7.0), look_at=(0.0, 1.0, 0.0), view_angle=40.0)


LAYOUT_FAMILIES = {
    "concentric": concentric, "collinear": collinear, "coplanar": coplanar,
    "big8": lambda w=16, h=9: big(8, w, h), "big9": lambda w=16, h=9: big(9, w, h), "uniform": uniform,
}
LAYOUT_FAMILIES.update({f"count{n}": (lambda n: lambda w=16, h=9: count(n, w, h))(n) for n in COUNTS})
