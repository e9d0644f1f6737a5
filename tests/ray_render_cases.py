"""Caller-supplied primary rays (rt_render_rays_async): the ray sets and the two references of
tests/test_ray_render_cases.py (no GPU) and tests/test_gpu_ray_render.py.

Reference A, the C oracle with a degenerate camera: vu = vv = du = dv = 0, center = o, ulc = target.  Camera::get_ray
then gives every sample the one ray (o, unit(target - o)) whatever its jitter draws, so oracle_render_{f64,f32} with
pixels = [pix] traces spp samples of that ray keyed by pix: one ray per pixel (R = 1).  unit is the oracle's
v / sqrt((x x + y y) + z z), which numpy reproduces exactly in float32 and float64 (unit_dirs).

Reference B, tests/independent_v2.trace_vectorized2 (imported, unchanged; the scene built with literal=True): the live
path restated in Python over packets of arbitrary per-sample primary rays, in fp64 and fp32.  Sample s of pixel p
starts as ray s % R of the pixel, and the draws are keyed by pix = pixel_base + p.
"""
import functools

import numpy as np

import independent_v2 as iv
import rt_mi355x as rt
from oracle_bind import oracle_render
from rt_mi355x import abi

PRECS = ("f64", "f32")
DTYPES = {"f64": np.float64, "f32": np.float32}
SEED = 0x5EED0001
PIXEL_BASE = 0x00A71000   # nonzero: the draws are keyed by pixel_base + p
N_PIX = 130               # two full batches of 64 lanes and a partial one


@functools.lru_cache(maxsize=None)
def scene(name):
    """"s100": rt.scenes.random_spheres(100), all three materials, no mega level; "mega": config E's 10 000 spheres."""
    return (rt.scenes.random_spheres(100) if name == "s100" else rt.scenes.config_scene("E")).flatten()


def unit_dirs(o, target):
    """unit(target - o) per row, in the arrays' type, as the oracle's get_ray computes it (no FMA, left to right)."""
    v = target - o
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return v / np.sqrt((x * x + y * y) + z * z)[:, None]


# centres of the three unit spheres of random_spheres (glass, lambertian, metal)
BIG = np.array([[0.0, 1.0, 0.0], [-4.0, 1.0, 0.0], [4.0, 1.0, 0.0]])
N_INSIDE, N_SKY = 6, 6


@functools.lru_cache(maxsize=None)
def ray_set(prec, n=N_PIX, seed=1):
    """n rays over the random scenes: (o, target, d = unit(target - o)) in the precision's type.  Rays 0 .. 5 start
    inside the three unit spheres, rays 6 .. 11 point up into the sky; the rest cross the field of small spheres."""
    rng = np.random.default_rng(seed)
    T = DTYPES[prec]
    o = np.stack([rng.uniform(-12, 12, n), rng.uniform(0.3, 6, n), rng.uniform(-12, 12, n)], 1)
    tgt = np.stack([rng.uniform(-8, 8, n), rng.uniform(0, 1.2, n), rng.uniform(-8, 8, n)], 1)
    o[:N_INSIDE] = np.repeat(BIG, 2, 0) + rng.uniform(-0.4, 0.4, (N_INSIDE, 3))
    sky = slice(N_INSIDE, N_INSIDE + N_SKY)
    o[sky, 1] = 3.0   # above every sphere but the ground's horizon
    tgt[sky] = o[sky] + np.stack([rng.uniform(-1, 1, N_SKY), np.full(N_SKY, 5.0), rng.uniform(-1, 1, N_SKY)], 1)
    o, tgt = o.astype(T), tgt.astype(T)
    d = unit_dirs(o, tgt)
    assert d.dtype == T
    for a in (o, tgt, d):
        a.setflags(write=False)
    return o, tgt, d


def degenerate_camera(o, target):
    cam = abi.RtCamera()
    cam.image_width = cam.image_height = 1
    for i in range(3):
        cam.center[i] = float(o[i])
        cam.ulc[i] = float(target[i])
    return cam


def reference_a(flat, o, target, spp, depth, prec, root2=False, seed=SEED, pixel_base=PIXEL_BASE):
    """Reference A over the rays (o[p], unit(target[p] - o[p])): (rgb [n, 3] u8, linear [n, 3] f64, segments, rc)."""
    n = o.shape[0]
    rgb, lin = np.zeros((n, 3), np.uint8), np.zeros((n, 3), np.float64)
    segs, rc = 0, 0
    for p in range(n):
        r, l, s, c = oracle_render(flat, degenerate_camera(o[p], target[p]), depth, spp, seed,
                                   abi.RT_FLAG_ROOT2 if root2 else 0, pixels=np.array([pixel_base + p], np.uint32),
                                   precision=prec, threads=1)
        rgb[p], lin[p] = r[0], l[0]
        segs += s
        rc = max(rc, c)
    return rgb, lin, segs, rc


def reference_b(flat, o, d, spp, depth, prec, seed=SEED, pixel_base=PIXEL_BASE):
    """Reference B.  o, d: [n, R, 3] in the precision's type.  Returns (rgb [n, 3] u8, linear [n, 3] f64, segments,
    rc): rc is RT_ERR_RANGE where a channel exceeds 2.0 (Color::to_u8_array panics; the image is still written, the
    byte saturating as `as u8` does)."""
    T = iv.F32 if prec == "f32" else float
    spheres, smat, mats = iv.scene_from_flat(flat, prec, literal=True)
    n, R = d.shape[0], d.shape[1]
    rgb, lin = np.zeros((n, 3), np.uint8), np.zeros((n, 3), np.float64)
    stats = {"segments": 0}
    code = abi.RT_OK

    def q8(v):   # color.rs:54-64 without the assert
        x = iv.sqrt(v) * 255.999
        return 0 if not x > 0.0 else 255 if x >= 255.0 else int(x)

    for p in range(n):
        chunks = []
        for s in range(spp):   # renderer.rs:157 .chunks(4), as independent_v2.render_pixel has it
            if s % iv.N == 0:
                pk = iv.Packet(T(0.0))
                pk.en = [False] * iv.N
                chunks.append(pk)
            ray = s % R
            pk.o[s % iv.N] = tuple(T(x) for x in o[p, ray])
            pk.d[s % iv.N] = tuple(T(x) for x in d[p, ray])
            pk.en[s % iv.N], pk.sid[s % iv.N] = True, s
        tot = iv.trace_vectorized2(spheres, smat, mats, chunks, depth, pixel_base + p, seed, stats, prec)
        val = tuple(t / spp for t in tot)
        lin[p] = [float(v) for v in val]
        rgb[p] = [q8(v) for v in val]
        if not all(v <= 2.0 for v in val):
            code = abi.RT_ERR_RANGE
    return rgb, lin, stats["segments"], code


def bound_lengths(T):
    """The shortest and the longest axis-direction lengths x the precondition admits in type T: x x (one rounding, what
    |d|^2 is for an axis direction) is the first value >= T(1e-6), the last <= T(1e6)."""
    lo, hi = T(1e-6), T(1e6)
    x = np.sqrt(lo)
    while x * x < lo:
        x = np.nextafter(x, T(1))
    while np.nextafter(x, T(0)) * np.nextafter(x, T(0)) >= lo:
        x = np.nextafter(x, T(0))
    y = np.sqrt(hi)
    while y * y > hi:
        y = np.nextafter(y, T(0))
    while np.nextafter(y, T(np.inf)) * np.nextafter(y, T(np.inf)) <= hi:
        y = np.nextafter(y, T(np.inf))
    return x, y


@functools.lru_cache(maxsize=None)
def per_sample_rays(prec, R, n=12, seed=7):
    """n pixels of R rays each, every ray on its own: origins over the field, directions of lengths between the
    bounds of the precondition; ray 0 of pixels 0 and 1 has |d|^2 exactly at the lower and the upper bound."""
    rng = np.random.default_rng(seed + R)
    T = DTYPES[prec]
    o = np.stack([rng.uniform(-10, 10, (n, R)), rng.uniform(0.3, 4, (n, R)), rng.uniform(-10, 10, (n, R))], -1)
    tgt = np.stack([rng.uniform(-6, 6, (n, R)), rng.uniform(0, 1.2, (n, R)), rng.uniform(-6, 6, (n, R))], -1)
    v = tgt - o
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v *= 10.0 ** rng.uniform(-2.5, 2.5, (n, R, 1))
    o, d = o.astype(T), v.astype(T)
    lo, hi = bound_lengths(T)
    d[0, 0] = [lo, 0, 0]
    d[1, 0] = [0, 0, -hi]
    for a in (o, d):
        a.setflags(write=False)
    return o, d
