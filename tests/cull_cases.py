"""Adversarial rays for the sweeps' culls (tests/test_cull_cases.py checks them on the CPU with the oracle alone,
tests/test_gpu_cull_probe.py runs them through the device's own nearest_hit and camera_sweep).

A case picks a target sphere (c, r) of a scene and aims a ray so that the centre's distance from the ray's line is
r (1 + s delta), s = +-1: the construction of tests/filter_margin_fuzz.c and its siblings, on the spheres of a real
scene image.  delta is log-uniform in [5e-10, 5e-4]; for fp64 rays two thirds of the cases draw it from [1e-17, 1e-13]
instead, the range in which only the reference's own rounding decides.  A ray is built in extended precision, its
origin rounded to the ray type T, and the direction then aimed again from the rounded origin, so the rounding of the
origin (large for the translated scene) does not move the line off the sphere.  Every case carries the delta its
rounded ray really has (measured in extended precision: |(c - o) x d| / (|d| r) - 1), which is what the shares in
tests/test_cull_cases.py are counted with.

Scenes: the smallest that reach each path of the sweep (their structure is asserted from build_scene_image's counts).
Families: graze, box_graze, near_equal, degenerate, camera.  Wave compositions: solo, full, mixed; camera also bundle.
Everything is seeded by (scene, family, precision): the CPU and the GPU test see the same rays.
"""
import functools
import zlib

import numpy as np

import rt_mi355x as rt
import devunit_bind as db
from oracle_bind import oracle_nearest_hit

LD = np.longdouble
WAVE = 64
N_CASES = 1024          # cases of a (scene, family): full 1024 lanes, mixed 3072, solo and bundle 16384 (the cap)
N_SOLO = 256            # cases the one-lane-per-wave compositions take (256 waves)
MAX_RAYS = 16384
N_POOL = 128            # distinct targets of a (scene, family)
SOLO_LANES = (0, 31, 32, 63)
MODES = ("packed", "root2", "scalar")
DTYPES = {"f32": np.float32, "f64": np.float64}
DELTA = (5e-10, 5e-4)
DELTA_F64 = (1e-17, 1e-13)
T_MIN = 0.001           # the reference's smallest valid root
P_OUTSIDE = 0.66        # the share of cases aimed outside their sphere (fp32's scalar mode accepts about half of them)
N_INNER = 8             # small spheres inside the shell sphere (scene indices 2 .. 9; the shell is 1, the ground 0)
SHELL = 1
N_PAIRS = 6             # pairs of crossing spheres in different clusters (near_equal)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _unit(v):
    return v / np.sqrt((v * v).sum(0))


def _dirs(rng, n):
    return _unit(rng.standard_normal((3, n)).astype(LD))


def _perp(rng, dhat):
    q = rng.standard_normal(dhat.shape).astype(LD)
    q = q - (q * dhat).sum(0) * dhat
    return _unit(q)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _round(v, dtype):
    """v in extended precision -> the values of dtype, kept in extended precision."""
    return v.astype(dtype).astype(LD)


# ---- scenes ----
class CullScene:
    def __init__(self, name, flat, half):
        self.name, self.flat, self.half = name, flat, half
        self.counts, self.ridx = db.scene_layout(flat)
        self.first = 1   # sphere 0 is the ground: never a target
        self.pairs = []
        self.mid = flat.center[1:].mean(0)

    def geom(self, dtype):
        """Centres [3, n] and radii [n] as the ray type holds them, in extended precision."""
        return self.flat.center.astype(dtype).astype(LD).T.copy(), self.flat.radius.astype(dtype).astype(LD)

    @functools.lru_cache(maxsize=None)
    def single(self, j):
        f = self.flat
        return rt.FlatScene(f.center[j:j + 1], f.radius[j:j + 1], [0], f.materials)

    def cluster_of(self):
        """Per scene index its cluster (-1: always exact)."""
        nx = 4 * self.counts["n_xg"]
        out = np.full(self.flat.n_spheres, -1, np.int64)
        slots = self.ridx[nx:]
        real = slots != 0xFFFFFFFF
        out[slots[real]] = (np.arange(slots.size) // 16)[real]
        return out

    def clusters(self):
        """Member scene indices of each cluster, from the slot table."""
        nx = 4 * self.counts["n_xg"]
        blocks = self.ridx[nx:].reshape(-1, 16)
        return [b[b != 0xFFFFFFFF].astype(np.int64) for b in blocks if (b != 0xFFFFFFFF).any()]


def _build(name, n, scale=1.0, shift=(0.0, 0.0, 0.0), wide_radii=False, pitch=None):
    """A ground sphere (always exact: |c|_1 + r far above 8x the median) and n spheres uniform in a box."""
    rng = _rng("scene", n, wide_radii)   # not the name: the translated scene is the same scene
    pitch = pitch or (3.0 if wide_radii else 1.6)
    half = 0.5 * pitch * n ** (1.0 / 3.0)
    cen = rng.uniform(-half, half, (n, 3))
    rad = 10.0 ** rng.uniform(-3.0, 0.0, n) if wide_radii else rng.uniform(0.05, 0.4, n)
    # spheres 1 .. N_INNER + 1: a shell and N_INNER small spheres inside it (the camera centre inside a sphere looks
    # at these: under root2 and scalar nothing beyond the shell can be the nearest hit)
    cen[0] = rng.uniform(-0.5 * half, 0.5 * half, 3)
    rad[0] = 0.42   # below kBigRatio x the median radius: the shell stays a cluster member
    cen[1:1 + N_INNER] = cen[0] + _unit(rng.standard_normal((3, N_INNER))).T * rng.uniform(0.15, 0.27, (N_INNER, 1))
    rad[1:1 + N_INNER] = rng.uniform(0.03, 0.06, N_INNER)
    local = np.vstack([[0.0, -half - 1001.0, 0.0], cen]) * scale
    cen = local + np.asarray(shift)
    rad = np.concatenate([[1000.0], rad]) * scale
    mats = [rt.Lambertian((0.5, 0.5, 0.5))]
    # near_equal's pairs: the closest spheres of different clusters (different supers where there are several) get
    # radii of 0.55 of their distance, so their surfaces cross.  The k-d layout depends on the centres alone.
    pre = CullScene(name, rt.FlatScene(cen, rad, np.zeros(n + 1, np.uint32), mats), half * scale)
    cl = pre.cluster_of()
    level = 4 if pre.counts["n_top"] > 1 else 1
    free = np.flatnonzero(cl >= 0)
    free = free[free >= 2 + N_INNER]
    dist = np.sqrt(((local[free, None, :] - local[None, free, :]) ** 2).sum(-1))   # before the shift: the same radii
    dist[(cl[free, None] // level) == (cl[None, free] // level)] = np.inf
    pairs, used = [], set()
    for flat_i in np.argsort(dist, axis=None)[:4000]:
        i, j = np.unravel_index(flat_i, dist.shape)
        a, b = int(free[i]), int(free[j])
        if a < b and a not in used and b not in used and dist[i, j] < 0.85 * scale * (3.0 if wide_radii else 1.0):
            pairs.append((a, b))
            used |= {a, b}
            rad[a] = rad[b] = 0.55 * dist[i, j]
        if len(pairs) == N_PAIRS:
            break
    flat = rt.FlatScene(cen, rad, np.zeros(n + 1, np.uint32), mats)
    sc = CullScene(name, flat, half * scale)
    sc.pairs = pairs
    return sc


# name -> (builder, the structure build_scene_image must give it)
SCENES = {
    "a_one_super": (lambda: _build("a_one_super", 39, pitch=1.1), dict(n_xs=1, n_top=1, n_mg=0)),
    "b_supers": (lambda: _build("b_supers", 299), dict(n_xs=1, n_top=8, n_mg=0)),
    "c_32_supers": (lambda: _build("c_32_supers", 2048), dict(n_xs=1, n_top=32, n_mg=0)),
    "d_mega": (lambda: _build("d_mega", 2600), dict(n_xs=1, n_mg=3, n_gg=1)),
    # the same spheres 5.8e3 extents away: the group-local and cluster-local frames carry the load
    "d_mega_far": (lambda: _build("d_mega_far", 2600, shift=(4e4, -7e4, 1e5)), dict(n_xs=1, n_mg=3, n_gg=1)),
    "e_scale_0.1": (lambda: _build("e_scale_0.1", 299, scale=0.1, wide_radii=True), dict(n_xs=1, n_top=8, n_mg=0)),
    "e_scale_1000": (lambda: _build("e_scale_1000", 299, scale=1000.0, wide_radii=True), dict(n_xs=1, n_top=8, n_mg=0)),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


# ---- rays ----
class Rays:
    """n rays: o, d [3, n] in the ray type; target [n] (-1: none); delta [n], the signed measured one (nan: none)."""

    def __init__(self, o, d, target=None, delta=None, centre=None, axis=None):
        n = d.shape[1]
        self.axis = axis   # box_graze: the box face's axis per ray
        self.o, self.d = np.ascontiguousarray(o), np.ascontiguousarray(d)
        self.target = np.full(n, -1, np.int64) if target is None else np.asarray(target, np.int64)
        self.delta = np.full(n, np.nan) if delta is None else np.asarray(delta, np.float64)
        self.centre = centre
        self.n = n

    def take(self, i):
        return Rays(self.o[:, i], self.d[:, i], self.target[i], self.delta[i], self.centre)


def measure(sc, dtype, o, d, target):
    """The signed delta of rounded rays against their targets: |(c - o) x d| / (|d| r) - 1, in extended precision."""
    C, r = sc.geom(dtype)
    w = C[:, target] - o.astype(LD)
    dd = d.astype(LD)
    x = np.stack([w[1] * dd[2] - w[2] * dd[1], w[2] * dd[0] - w[0] * dd[2], w[0] * dd[1] - w[1] * dd[0]])
    dist = np.sqrt((x * x).sum(0)) / np.sqrt((dd * dd).sum(0))
    return (dist / r[target] - 1).astype(np.float64)


def _aim(C, O, rho, q):
    """Unit directions from O whose line passes the points C at distance rho (bent towards q)."""
    w = C - O
    D = np.sqrt((w * w).sum(0))
    u = w / D
    qp = q - (q * u).sum(0) * u
    qp = _unit(qp)
    s = np.minimum(rho / D, LD(1))
    return np.sqrt(1 - s * s) * u + s * qp


def _deltas(rng, dtype, n):
    sign = np.where(rng.random(n) < P_OUTSIDE, 1.0, -1.0)
    delta = _logu(rng, *DELTA, n)
    if dtype == np.float64:
        small = rng.random(n) < 0.65
        delta = np.where(small, _logu(rng, *DELTA_F64, n), delta)
    return sign.astype(LD) * delta.astype(LD)


def _dscale(rng, n):
    """Direction lengths: unit, or 1e-3 .. 1e3."""
    return np.where(rng.random(n) < 0.5, 1.0, _logu(rng, 1e-3, 1e3, n)).astype(LD)


def _g_range(r, grid=None):
    """The origin's distance from the surface, in radii: 1e-2 .. 1e3, and far enough for a valid root (t >= 2 t_min).
    grid: the ray type's spacing at the origin; box_graze keeps the origin 1024 of them away, so that its rounding
    tilts the ray by less than 1e-3."""
    lo = np.maximum(1e-2, np.sqrt(1 + (2 * T_MIN / r.astype(np.float64)) ** 2) - 1)
    if grid is not None:
        lo = np.maximum(lo, 1024 * (grid / r).astype(np.float64))
    return lo, np.maximum(1e3, 2 * lo)


def graze(sc, dtype):
    rng = _rng(sc.name, "graze", np.dtype(dtype).name)
    C, r = sc.geom(dtype)
    n = N_CASES
    pool = rng.choice(np.arange(sc.first, r.size), min(N_POOL, r.size - sc.first), replace=False)
    tgt = pool[rng.integers(pool.size, size=n)]
    Ct, rt_ = C[:, tgt], r[tgt]
    rho = rt_ * (1 + _deltas(rng, dtype, n))
    dhat = _dirs(rng, n)
    near_axis = rng.random(n) < 0.25   # near an axis: one component dominates by 1e4 .. 1e9
    ax = rng.integers(3, size=n)
    e = np.zeros((3, n), LD)
    e[ax, np.arange(n)] = rng.choice([-1.0, 1.0], n)
    dhat = np.where(near_axis, _unit(e + dhat * _logu(rng, 1e-9, 1e-4, n).astype(LD)), dhat)
    phat = _perp(rng, dhat)
    lo, hi = _g_range(rt_)
    g = np.exp(rng.uniform(np.log(lo), np.log(hi))).astype(LD)
    L = np.sqrt(np.maximum((rt_ * (1 + g)) ** 2 - rho ** 2, 0))
    O = _round(Ct - L * dhat - rho * phat, dtype)
    d = (_aim(Ct, O, rho, -phat) * _dscale(rng, n)).astype(dtype)
    o = O.astype(dtype)
    return Rays(o, d, tgt, measure(sc, dtype, o, d, tgt))


# signed |d_a| values around nearest_hit's 1e-20 clamp of the slab test's 1/d
CLAMP_VALUES = (0.0, -0.0, 1e-21, -1e-21, 1e-20, -1e-20, 1e-19, -1e-19)
TILTS = (0.0, 1e-7, 1e-3)


def box_graze(sc, dtype):
    """Targets that set their cluster box's extent on an axis, touched at that extreme point by rays that run nearly
    parallel to the box face.  A quarter of the rays hold one of CLAMP_VALUES in the face's axis exactly (their
    origin's coordinate on that axis is rounded, not aimed again); the others tilt by one of TILTS and are aimed
    through the point c + r (1 + s delta) e_a from the rounded origin."""
    rng = _rng(sc.name, "box_graze", np.dtype(dtype).name)
    C, r = sc.geom(dtype)
    n = N_CASES
    trip = []   # (target, axis, side)
    for mem in sc.clusters():
        mem = mem[mem >= sc.first]
        if mem.size == 0:
            continue
        for a in range(3):
            trip.append((mem[np.argmax(C[a, mem] + r[mem])], a, 1.0))
            trip.append((mem[np.argmin(C[a, mem] - r[mem])], a, -1.0))
    trip = np.array(trip, dtype=object)
    trip = trip[rng.choice(len(trip), min(N_POOL, len(trip)), replace=False)]
    pick = rng.integers(len(trip), size=n)
    tgt = trip[pick, 0].astype(np.int64)
    ax = trip[pick, 1].astype(np.int64)
    side = trip[pick, 2].astype(np.float64).astype(LD)
    Ct, rt_ = C[:, tgt], r[tgt]
    cols = np.arange(n)
    ea = np.zeros((3, n), LD)
    ea[ax, cols] = 1
    tilt = rng.choice(TILTS, n).astype(LD) * rng.choice([-1.0, 1.0], n)
    # the aim point: the line through it along dhat + tilt e_a passes c at r (1 + s delta)
    E = Ct + ea * (side * rt_ * (1 + _deltas(rng, dtype, n)) * np.sqrt(1 + tilt * tilt))
    dhat = _dirs(rng, n)
    aligned = rng.random(n) < 0.25   # along another axis: two zero components
    e2 = np.zeros((3, n), LD)
    e2[(ax + 1 + rng.integers(2, size=n)) % 3, cols] = rng.choice([-1.0, 1.0], n)
    dhat = np.where(aligned, e2, dhat)
    dhat = dhat - ea * (dhat * ea).sum(0)
    dhat = _unit(dhat)                 # in the face's plane
    lo, hi = _g_range(rt_, np.finfo(dtype).eps * np.abs(Ct).max(0))
    L = rt_ * np.exp(rng.uniform(np.log(lo), np.log(hi))).astype(LD)
    O = _round(E - L * (dhat + ea * tilt), dtype)
    w = E - O
    d = w / np.sqrt((w * w).sum(0))    # aimed again through E
    exact = rng.random(n) < 0.25
    da = rng.choice(CLAMP_VALUES, n).astype(LD)
    d = np.where(exact, dhat, d) * _dscale(rng, n)
    d = d.astype(dtype)
    d[ax[exact], cols[exact]] = da[exact].astype(dtype)
    o = O.astype(dtype)
    return Rays(o, d, tgt, measure(sc, dtype, o, d, tgt), axis=ax)


def degenerate(sc, dtype, n=N_CASES, seed="degenerate"):
    """No grazing: directions within 1e-8 of +-y (the filter's zero basis), origins with |o|_1 around 1e15, zero
    components in d; each aimed at some sphere, so most of them hit."""
    rng = _rng(sc.name, seed, np.dtype(dtype).name)
    C, r = sc.geom(dtype)
    tgt = rng.integers(sc.first, r.size, size=n)
    Ct, rt_ = C[:, tgt], r[tgt]
    kind = np.arange(n) % 3
    cols = np.arange(n)
    # 0: along +-y within 1e-8
    dy = np.zeros((3, n), LD)
    dy[1] = rng.choice([-1.0, 1.0], n)
    dy[0] = rng.uniform(-1e-8, 1e-8, n)
    dy[2] = rng.uniform(-1e-8, 1e-8, n)
    # 1: any direction, from 3e14 .. 3e15 away
    dfar = _dirs(rng, n)
    # 2: one or two zero components
    dz = _dirs(rng, n)
    z1 = rng.integers(3, size=n)
    dz[z1, cols] = 0
    z2 = (z1 + 1 + rng.integers(2, size=n)) % 3
    dz[z2, cols] = np.where(rng.random(n) < 0.5, 0, dz[z2, cols])
    dz = np.where((dz * dz).sum(0) == 0, dy, dz)
    dhat = _unit(np.where(kind == 0, dy, np.where(kind == 1, dfar, dz)))
    L = np.where(kind == 1, _logu(rng, 3e14, 3e15, n), rt_.astype(np.float64) * _logu(rng, 1.5, 100.0, n)).astype(LD)
    off = _perp(rng, dhat) * rt_ * rng.uniform(0.0, 1.2, n).astype(LD)
    o = (Ct - L * dhat + off).astype(dtype)
    d = (dhat * _dscale(rng, n)).astype(dtype)
    d[0, kind == 0] = dy[0, kind == 0].astype(dtype)   # the small components as drawn (|d_y| = 1 for these)
    d[2, kind == 0] = dy[2, kind == 0].astype(dtype)
    d[1, kind == 0] = dy[1, kind == 0].astype(dtype)
    d = np.where(np.abs(dhat) == 0, dtype(0), d)       # zero components stay zero
    return Rays(o, d)


def root_pair(sc, mode, rays, a, b):
    """The reference's roots of spheres a and b alone, and their difference in ulp (nan roots: no valid root)."""
    ia, ta = oracle_nearest_hit(sc.single(a), mode, rays.o, rays.d)
    ib, tb = oracle_nearest_hit(sc.single(b), mode, rays.o, rays.d)
    bits = np.int32 if ta.dtype == np.float32 else np.int64
    ulp = ta.view(bits).astype(np.int64) - tb.view(bits).astype(np.int64)   # positive roots order as their bits
    return (ia == 0) & (ib == 0), ulp


def near_equal(sc, dtype):
    """Rays through the circle in which the surfaces of two spheres of different clusters (sc.pairs) cross, entering
    both there, so the two roots agree to a few ulp: the box-time bound tn <= bt against the tie rule.  Around each
    such ray, aimed in extended precision from its rounded origin, the directions whose first two components lie
    up to 3 ulp away are tried in the oracle's own arithmetic, and those are kept whose roots differ by at most 4 ulp
    in some mode (the rays of the ray type are discrete: stepping through them is the bisection's last stage)."""
    rng = _rng(sc.name, "near_equal", np.dtype(dtype).name)
    C, r = sc.geom(dtype)
    o_all, d_all, pair_all = [], [], []
    for pi, (a, b) in enumerate(sc.pairs):
        n = (C[:, b] - C[:, a])
        D = np.sqrt((n * n).sum())
        n = n / D
        x = (D * D + r[a] * r[a] - r[b] * r[b]) / (2 * D)
        h2 = r[a] * r[a] - x * x
        if not h2 > 0:
            continue
        for _ in range(8):
            e = _perp(rng, n[:, None])[:, 0]
            X = C[:, a] + x * n + np.sqrt(h2) * e
            w = X[:, None] - C
            if ((w * w).sum(0) < r * r * (1 - 1e-6)).sum() > 0:   # inside a third sphere
                continue
            dh = -_unit(((X - C[:, a]) / r[a] + (X - C[:, b]) / r[b])[:, None])[:, 0]
            dh = _unit((dh + 0.25 * _dirs(rng, 1)[:, 0])[:, None])[:, 0]
            if not (dh @ (X - C[:, a]) < 0 and dh @ (X - C[:, b]) < 0):
                continue
            O = _round(X - dh * (r[a] * LD(rng.uniform(0.5, 5.0))), dtype)
            # bisection in the oracle's arithmetic: slide the aim point X + s g towards a's side until the two roots
            # change order (the centres' own rounding moves the crossing by far more than an ulp of t)
            g = C[:, a] - C[:, b]
            g = _unit((g - (g @ dh) * dh)[:, None])[:, 0]
            dl = _dscale(rng, 1)[0]
            XO = X - O   # small: sliding by s g stays resolved however far the scene lies from the origin
            aim = lambda sv: (_unit((XO + sv * g)[:, None])[:, 0] * dl).astype(dtype)   # noqa: E731

            def order(sv):
                one = Rays(O.astype(dtype)[:, None], aim(sv)[:, None])
                ok, ulp = root_pair(sc, "packed", one, a, b)
                return int(ulp[0]) if ok[0] else None
            lo, hi = -1e-4 * r[a], 1e-4 * r[a]
            flo, fhi = order(lo), order(hi)
            if flo is None or fhi is None or (flo > 0) == (fhi > 0):
                continue
            for _ in range(70):
                mid = (lo + hi) / 2
                fm = order(mid)
                if fm is None:
                    break
                if (fm > 0) == (flo > 0):
                    lo = mid
                else:
                    hi = mid
            d0 = aim(lo)
            i1, i2 = rng.permutation(3)[:2]
            for k1 in range(-3, 4):
                for k2 in range(-3, 4):
                    d = d0.copy()
                    for i, k in ((i1, k1), (i2, k2)):
                        for _ in range(abs(k)):
                            d[i] = np.nextafter(d[i], dtype(np.inf if k > 0 else -np.inf))
                    o_all.append(O.astype(dtype))
                    d_all.append(d)
                    pair_all.append(pi)
    rays = Rays(np.array(o_all, dtype).T, np.array(d_all, dtype).T)
    pair = np.array(pair_all)
    keep = np.zeros(rays.n, bool)
    for mode in MODES:
        for pi, (a, b) in enumerate(sc.pairs):
            m = np.flatnonzero(pair == pi)
            if m.size:
                ok, ulp = root_pair(sc, mode, rays.take(m), a, b)
                keep[m[ok & (np.abs(ulp) <= 4)]] = True
    idx = np.flatnonzero(keep)
    assert idx.size >= 16, (sc.name, idx.size)
    idx = np.resize(idx, N_CASES)   # cycled up to whole blocks
    out = rays.take(idx)
    out.pair = pair[idx]
    return out


def misses(sc, dtype, n, centre=None):
    """Rays that leave the scene upwards from above it (the ground lies below); camera: upwards from the centre."""
    rng = _rng(sc.name, "miss", np.dtype(dtype).name)
    d = _dirs(rng, n)
    d[1] = np.abs(d[1]) + 0.2
    o = np.asarray(sc.mid, np.float64)[:, None] + sc.half * np.vstack([rng.uniform(-1, 1, n), rng.uniform(2.5, 4, n),
                                                                       rng.uniform(-1, 1, n)])
    return Rays(o.astype(dtype), (d * _dscale(rng, n)).astype(dtype))


def random_rays(sc, dtype, n=4096):
    """Plain rays (the control): origins in and around the scene's box, any direction."""
    rng = _rng(sc.name, "random", np.dtype(dtype).name)
    o = np.asarray(sc.mid, np.float64)[:, None] + sc.half * rng.uniform(-1.5, 1.5, (3, n))
    return Rays(o.astype(dtype), rng.standard_normal((3, n)).astype(dtype))


# ---- camera ----
CENTRES = ("outside_0", "outside_1", "inside", "on")


def _candidates(sc, C, r, P, anchor, which):
    """The camera targets of centre P: spheres 1.05 .. 15 radii away.  inside: the spheres inside the shell.  on: those
    on the outer side of the centre's sphere, so that a ray grazing them does not enter it."""
    w = C - P[:, None]
    wn = np.sqrt((w * w).sum(0))
    k = (wn / r).astype(np.float64)
    ok = (k >= 1.05) & (k <= 15)
    ok[:sc.first] = False
    if which == "inside":
        ok[:SHELL + 1] = False
        ok[SHELL + 1 + N_INNER:] = False
    if which == "on":
        nrm = _unit(P - C[:, anchor])
        ok &= ((w * nrm[:, None]).sum(0) / wn).astype(np.float64) > 1 / np.maximum(k, 1.0) + 0.05
    return np.flatnonzero(ok)


@functools.lru_cache(maxsize=None)
def _centre(name, prec, which):
    sc, dtype = scene(name), DTYPES[prec]
    rng = _rng(sc.name, "centre", which, prec)
    C, r = sc.geom(dtype)
    best = None
    for _ in range(400):
        j = SHELL if which == "inside" else int(rng.integers(sc.first, r.size))
        u = _dirs(rng, 1)[:, 0]
        k = {"inside": LD(rng.uniform(0.0, 0.25)), "on": LD(1)}.get(which, LD(rng.uniform(1.5, 4.0)))
        p = (C[:, j] + k * r[j] * u).astype(dtype)
        if which == "on":   # the reference's c in the ray type; step towards the sphere's centre until it is <= 0
            cj, r2 = C[:, j].astype(dtype), r[j].astype(dtype) * r[j].astype(dtype)
            for _ in range(64):
                if ref_c(p - cj, r2) <= 0:
                    break
                p = np.nextafter(p, cj)
        w = p.astype(LD)[:, None] - C
        inside = set(np.flatnonzero((w * w).sum(0) <= r * r).tolist())
        if inside != ({j} if which == "inside" else set()) and not (which == "on" and inside <= {j}):
            continue
        if which == "on":   # on or at most 0.0004 below the surface: leaving the sphere is no valid root (t < t_min)
            c = float(ref_c(p - C[:, j].astype(dtype), r[j].astype(dtype) * r[j].astype(dtype)))
            if not (c <= 0 and -c <= 2 * float(r[j]) * 0.0004):
                continue
        cand = _candidates(sc, C, r, p.astype(LD), j, which)
        if best is None or cand.size > best[2].size:
            best = (p, j, cand)
        if cand.size >= 12 or (which == "inside" and cand.size >= 6):
            break
    assert best is not None and best[2].size >= 4, f"{sc.name}: no {which} centre"
    return best


def ref_c(oc, r2):
    """The reference's c = |oc|^2 - r^2 (scalar form) in the type of oc."""
    t = oc.dtype.type
    return t(t(t(oc[0] * oc[0]) + t(oc[1] * oc[1])) + t(oc[2] * oc[2])) - r2


def camera_centre(sc, dtype, which):
    """A camera centre in the ray type, its anchor sphere and its targets.  outside_*: outside every sphere, 1.5 .. 4
    radii from the anchor; inside: in the shell sphere only; on: on the anchor (the reference's c <= 0 in the ray
    type's arithmetic, as near the surface as the type gets).  Of up to 400 draws the first with 12 targets."""
    return _centre(sc.name, np.dtype(dtype).name.replace("float", "f"), which)


def camera(sc, dtype, which):
    """Directions from one centre that graze the silhouettes of the spheres 1.05 .. 15 radii away: rp's relative
    margin over r grows with (|w| / r)^2, so near spheres test it hardest."""
    rng = _rng(sc.name, "camera", which, np.dtype(dtype).name)
    C, r = sc.geom(dtype)
    P, anchor, cand = camera_centre(sc, dtype, which)
    Pl = P.astype(LD)[:, None]
    # prefer the targets the centre sees: the ray to their centre hits them first
    aimed = Rays(np.repeat(P[:, None], cand.size, 1), (C[:, cand] - Pl).astype(dtype))
    seen = cand[oracle_nearest_hit(sc.flat, "packed", aimed.o, aimed.d)[0] == cand]
    if seen.size >= 4:
        cand = seen
    pool = rng.choice(cand, min(N_POOL, cand.size), replace=False)
    n = N_CASES
    tgt = pool[rng.integers(pool.size, size=n)]
    rho = r[tgt] * (1 + _deltas(rng, dtype, n))
    d = (_aim(C[:, tgt], np.repeat(Pl, n, 1), rho, _dirs(rng, n)) * _dscale(rng, n)).astype(dtype)
    o = np.repeat(P[:, None], n, 1)
    return Rays(o, d, tgt, measure(sc, dtype, o, d, tgt), centre=P)


def camera_fill(sc, dtype, P, n, seed):
    """Degenerate directions from the centre: within 1e-8 of +-y, and with zero components."""
    rng = _rng(sc.name, seed, np.dtype(dtype).name)
    d = _dirs(rng, n).astype(np.float64)
    kind = np.arange(n) % 2
    d[1] = np.where(kind == 0, np.sign(d[1]), d[1])
    d[0] = np.where(kind == 0, rng.uniform(-1e-8, 1e-8, n), d[0])
    d[2] = np.where(kind == 0, rng.uniform(-1e-8, 1e-8, n), d[2])
    z = rng.integers(3, size=n)
    d[z, np.arange(n)] = np.where(kind == 1, 0.0, d[z, np.arange(n)])
    return Rays(np.repeat(P[:, None], n, 1), d.astype(dtype), centre=P)


def family(sc, name, dtype):
    """name: graze, box_graze, degenerate, or camera:<centre>."""
    if name.startswith("camera:"):
        return camera(sc, dtype, name.split(":")[1])
    return {"graze": graze, "box_graze": box_graze, "degenerate": degenerate, "near_equal": near_equal}[name](sc, dtype)


GENERAL_FAMILIES = ("graze", "box_graze", "near_equal", "degenerate")
CAMERA_FAMILIES = tuple(f"camera:{c}" for c in CENTRES)
COMPOSITIONS = ("solo", "full", "mixed")
CAMERA_COMPOSITIONS = ("solo", "bundle", "full", "mixed")   # full: 64 unrelated silhouettes, a spread beyond 60 degrees


# ---- wave compositions ----
class Launch:
    """What a probe call takes: rays per lane, the active mask, and per lane the case's target and delta."""

    def __init__(self, rays, active, lane_case):
        self.rays, self.active, self.lane_case = rays, np.asarray(active, np.uint8), lane_case
        assert rays.n % db.BLOCK == 0 and rays.n <= MAX_RAYS


def compose(sc, fam, dtype, kind):
    """solo: one active lane per wave, at lane 0, 31, 32, 63 in turn, the only composition in which a lane's own box
    test, wave-level filter pass and cone decide alone.  full: 64 unrelated cases per wave.  mixed: every case
    between a degenerate lane and a lane that misses everything.  bundle (camera): each wave a tight bundle (1e-5
    of the direction's length) around one case."""
    rays = family(sc, fam, dtype)
    rng = _rng(sc.name, fam, np.dtype(dtype).name, kind)
    cam = rays.centre is not None
    if kind == "solo":
        m = N_SOLO
        pick = np.repeat(np.arange(m), WAVE)
        active = np.zeros(m * WAVE, np.uint8)
        active[np.arange(m) * WAVE + np.array(SOLO_LANES)[np.arange(m) % 4]] = 1
        return Launch(rays.take(pick), active, pick)
    if kind == "full":
        pick = rng.permutation(rays.n)
        return Launch(rays.take(pick), np.ones(rays.n, np.uint8), pick)
    if kind == "mixed":
        n = rays.n
        if cam:
            deg = camera_fill(sc, dtype, rays.centre, n, "mixed-degenerate")
            mis = misses(sc, dtype, n)
            mis = Rays(rays.o, mis.d, centre=rays.centre)
        else:
            deg = degenerate(sc, dtype, n, "mixed-degenerate")
            mis = misses(sc, dtype, n)
        pick = rng.permutation(n)
        g = rays.take(pick)
        il = lambda a, b, c: np.stack([a, b, c], -1).reshape(a.shape[:-1] + (3 * n,))   # noqa: E731
        out = Rays(il(g.o, deg.o, mis.o), il(g.d, deg.d, mis.d), il(g.target, deg.target, mis.target),
                   il(g.delta, deg.delta, mis.delta), rays.centre)
        return Launch(out, np.ones(3 * n, np.uint8), il(pick, np.full(n, -1), np.full(n, -1)))
    if kind == "bundle":
        assert cam
        m = N_SOLO
        pick = np.repeat(np.arange(m), WAVE)
        g = rays.take(pick)
        dl = np.sqrt((g.d.astype(np.float64) ** 2).sum(0))
        jit = rng.standard_normal((3, m * WAVE)) * 1e-5 * dl
        jit[:, np.arange(m) * WAVE + rng.integers(WAVE, size=m)] = 0   # one lane keeps the case's own direction
        d = (g.d.astype(np.float64) + jit).astype(dtype)
        out = Rays(g.o, d, g.target, measure(sc, dtype, g.o, d, g.target), rays.centre)
        return Launch(out, np.ones(m * WAVE, np.uint8), pick)
    raise KeyError(kind)


# ---- the reference ----
def reference(sc, mode, rays, active=None):
    """oracle_nearest_hit for the active rays; the inactive lanes hold the probe's untouched values."""
    idx = np.full(rays.n, db.IDX_UNTOUCHED, np.int32)
    t = np.full(rays.n, db.T_UNTOUCHED, rays.d.dtype)
    m = np.ones(rays.n, bool) if active is None else np.asarray(active, bool)
    idx[m], t[m] = oracle_nearest_hit(sc.flat, mode, rays.o[:, m], rays.d[:, m])
    return idx, t


def accepts(sc, mode, rays):
    """Per ray with a target: does the reference, given the target alone, report a hit (its own discriminant >= 0
    and a valid root)?"""
    acc = np.zeros(rays.n, bool)
    for j in np.unique(rays.target[rays.target >= 0]):
        m = rays.target == j
        idx, _ = oracle_nearest_hit(sc.single(int(j)), mode, rays.o[:, m], rays.d[:, m])
        acc[m] = idx == 0
    return acc
