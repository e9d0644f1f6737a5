"""Ray queries (rt_query_hits_async): the launches and the restatements tests/test_query_abi.py (CPU: the launches
checked with the oracle alone) and tests/test_gpu_query.py (GPU: query_rays<T, ROOT2, SHARED, MEGA> against them) share.

Plain module: no GPU, no fixtures.  tests/cull_cases.py (the adversarial rays of the sweeps' probe), tests/independent_v2.py
(the pure-Python restatement of the live path) and tests/edge_scenes.py are imported, not modified.

A launch is what one query takes: origins and directions [n, 3] in the ray type, the lanes the precondition leaves
valid, and per mode ("packed": quirk Q1 as the reference has it; "root2": RT_FLAG_ROOT2) the expected (index, t):
oracle_nearest_hit, brute force over every sphere in scene order, for the valid lanes, and (-2, NaN) for the others.
Every reference is computed once per key and left unchanged (read-only arrays).
"""
import functools

import numpy as np

import cull_cases as cc
import independent_v2 as iv
from oracle_bind import oracle_nearest_hit
from rt_mi355x import abi

SCENES = ("a_one_super", "b_supers", "d_mega", "d_mega_far")
FAMILIES = ("graze", "near_equal", "degenerate", "camera:outside_0", "camera:inside")
KINDS = ("full", "mixed", "solo")
MODES = ("packed", "root2")
PRECS = ("f64", "f32")
LEN2_MIN, LEN2_MAX = 1e-6, 1e6   # include/rt_mi355x.h: |d|^2 outside [1e-6, 1e6] (rounded to T) is invalid
MISS, INVALID = abi.RT_QUERY_MISS, abi.RT_QUERY_INVALID


def bits(a):
    """The bit patterns of a float array (NaN and inf patterns compare like any other)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def scalar_type(dtype):
    """The scalar arithmetic of independent_v2 for a ray type: numpy.float32 scalars, or Python floats."""
    return iv.F32 if np.dtype(dtype) == np.float32 else float


def valid_rays(o, d):
    """The precondition of include/rt_mi355x.h restated: every component finite and PackedVec3::length_squared of d,
    in the ray type (independent_v2's pk_len2: exact mul_add), inside [1e-6, 1e6] with the bounds rounded to the type.
    o: [n, 3] or [3] (a shared origin); d: [n, 3]."""
    d = np.asarray(d)
    T = scalar_type(d.dtype)
    lo, hi = T(d.dtype.type(LEN2_MIN)), T(d.dtype.type(LEN2_MAX))
    o = np.broadcast_to(np.asarray(o, dtype=d.dtype), d.shape)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    for i in np.flatnonzero(ok):
        a = iv.pk_len2(tuple(T(x) for x in d[i]))
        ok[i] = bool(lo <= a <= hi)
    return ok


def valid_fast(o, d):
    """valid_rays for rays whose |d|^2 is nowhere near a bound (asserted): no per-ray Python arithmetic."""
    d = np.asarray(d)
    o = np.broadcast_to(np.asarray(o, dtype=d.dtype), d.shape)
    fin = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    with np.errstate(all="ignore"):
        a = (d.astype(np.float64) ** 2).sum(1)
    near = fin & ((np.abs(a / LEN2_MIN - 1) < 1e-3) | (np.abs(a / LEN2_MAX - 1) < 1e-3))
    ok = fin & (a > LEN2_MIN) & (a < LEN2_MAX)
    if near.any():
        ok[near] = valid_rays(o[near], d[near])
    return ok


def with_coverage(sc, fam, dtype, la):
    """cull_cases' composition, unchanged, followed by whole waves of plain rays, so that no launch is made of hits
    alone and every target sphere can be reached: for a family with targets, one ray per case from the case's origin
    straight at its target's centre (1024 rays: the grazing rays of a target may all pass outside it, and rightly
    miss); then one wave of cull_cases.misses (a camera family's from its centre).  Returns (Rays, active)."""
    base = cc.family(sc, fam, dtype)
    parts, active = [la.rays], [np.asarray(la.active, bool)]
    if (base.target >= 0).all():
        C, _ = sc.geom(dtype)
        d = (C[:, base.target] - base.o.astype(cc.LD)).astype(dtype)
        parts.append(cc.Rays(base.o, d, base.target, centre=base.centre))
        active.append(np.ones(base.n, bool))
    mis = cc.misses(sc, dtype, cc.WAVE)
    if base.centre is not None:
        mis = cc.Rays(np.repeat(base.centre[:, None], cc.WAVE, 1), mis.d, centre=base.centre)
    parts.append(mis)
    active.append(np.ones(cc.WAVE, bool))
    rays = cc.Rays(np.concatenate([p.o for p in parts], 1), np.concatenate([p.d for p in parts], 1),
                   np.concatenate([p.target for p in parts]), centre=base.centre)
    return rays, np.concatenate(active)


class QueryLaunch:
    """One query: o, d [n, 3] in the ray type (centre: the shared origin of a camera family, else None), valid [n],
    target [n] (the sphere a lane's ray was aimed at, -1: none), and ref[mode] = (index [n] int32, t [n])."""

    def __init__(self, sc, rays, active):
        self.sc = sc
        self.o = np.ascontiguousarray(rays.o.T)
        self.centre = None if rays.centre is None else np.ascontiguousarray(rays.centre)
        d = np.ascontiguousarray(rays.d.T).copy()
        d[~np.asarray(active, bool)] = np.nan   # solo: NaN-direction lanes around the one valid lane of each wave
        self.d = d
        self.n = d.shape[0]
        self.valid = valid_fast(self.o, self.d)
        self.target = np.where(self.valid, rays.target, -1)
        self.ref = {}
        for mode in MODES:
            idx = np.full(self.n, INVALID, np.int32)
            t = np.full(self.n, np.nan, d.dtype)
            v = self.valid
            idx[v], t[v] = oracle_nearest_hit(sc.flat, mode, rays.o[:, v], rays.d[:, v])
            idx.setflags(write=False)
            t.setflags(write=False)
            self.ref[mode] = (idx, t)
        for a in (self.o, self.d, self.valid, self.target):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def launch(name, fam, prec, kind):
    sc = cc.scene(name)
    la = cc.compose(sc, fam, cc.DTYPES[prec], kind)
    return QueryLaunch(sc, *with_coverage(sc, fam, cc.DTYPES[prec], la))


# ---------------------------------------------------------------- finalize, restated
def finalize(flat, o, d, index, t):
    """PackedHitRecords::finalize (objects.rs:157-162) for rays whose closest hit (index, t) is known, on
    independent_v2's primitives: point = o + d t without FMA, normal = (point - centre) / sqrt(pk_len2(..)),
    front = pk_dot(d, normal) < 0, the normal negated when not front.  A miss or an invalid ray: zeros.
    Returns (normal [n, 3], point [n, 3], front [n] uint8) in the ray type."""
    d = np.asarray(d)
    dtype = d.dtype
    T = scalar_type(dtype)
    o = np.broadcast_to(np.asarray(o, dtype=dtype), d.shape)
    cen = flat.center.astype(dtype)
    n = d.shape[0]
    normal, point, front = np.zeros((n, 3), dtype), np.zeros((n, 3), dtype), np.zeros(n, np.uint8)
    for i in np.flatnonzero(np.asarray(index) >= 0):
        oo, dd = tuple(T(x) for x in o[i]), tuple(T(x) for x in d[i])
        c = tuple(T(x) for x in cen[index[i]])
        loc = iv.v_add(oo, iv.v_mul(dd, T(t[i])))
        vec = iv.v_sub(loc, c)
        u = iv.v_div(vec, iv.sqrt(iv.pk_len2(vec)))
        f = iv.pk_dot(dd, u) < 0.0
        if not f:
            u = iv.v_neg(u)
        normal[i], point[i], front[i] = u, loc, int(f)
    return normal, point, front


def restate_packed(flat, o, d, prec):
    """The whole definition under quirk Q1 from independent_v2.hit_scene (the object loop, update, finalize):
    (index, t, normal, point, front) for valid rays."""
    d = np.asarray(d)
    dtype = d.dtype
    T = scalar_type(dtype)
    o = np.broadcast_to(np.asarray(o, dtype=dtype), d.shape)
    spheres, _, _ = iv.scene_from_flat(flat, prec)
    n = d.shape[0]
    index, t = np.full(n, MISS, np.int32), np.full(n, np.inf, dtype)
    normal, point, front = np.zeros((n, 3), dtype), np.zeros((n, 3), dtype), np.zeros(n, np.uint8)
    for i in range(n):
        rec = iv.hit_scene(spheres, tuple(T(x) for x in o[i]), tuple(T(x) for x in d[i]))
        if rec is not None:
            t[i], point[i], normal[i], f, index[i] = rec
            front[i] = int(f)
    return index, t, normal, point, front


def assert_same(got, want, what=""):
    """0 ulp: the same bits, NaN and inf patterns and the sign of zero included."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what + " (bit patterns)")


# ---------------------------------------------------------------- pixel-centre rays (rt-render --pick, tools/query_ab.py)
def pixel_centre_rays(cam, pixels, dtype):
    """The rays rt-render --pick traces: Camera::get_ray (ray_tracing.rs:77-84) with both jitter draws at 0.5 and no
    defocus offset, in the ray type, every operation rounded once and none fused.  pixels: [(col, row)].
    Returns (origin [3] float64, directions [n, 3])."""
    t = np.dtype(dtype).type
    W, H = t(cam.image_width), t(cam.image_height)
    vu, vv, ulc, cen = ([t(x) for x in v] for v in (cam.vu, cam.vv, cam.ulc, cam.center))
    out = np.zeros((len(pixels), 3), dtype)
    for k, (col, row) in enumerate(pixels):
        fx, fy = (t(col) + t(0.5)) / W, (t(row) + t(0.5)) / H
        v = [(ulc[a] + (vu[a] * fx + vv[a] * fy)) - cen[a] for a in range(3)]
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        out[k] = [x / ln for x in v]
    return np.array(list(cam.center), np.float64), out
