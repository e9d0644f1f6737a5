"""Inputs and references of the next-ray stage's tests: the lanes tests/test_gpu_scatter.py runs through the product's
next_ray<T, SCALAR> (tests/device/rt_devunit.hip's next-ray probe), their reference (the oracle's next-ray and get-ray
probes) and a second, per-lane Python reference built from tests/independent_v2.py's primitives, which also takes the
mutations tests/test_scatter_cases.py checks the families against.

Plain module: no GPU, deterministic builders, fixed numpy seeds.  A family is a list of launches (one camera each) of
at most 4 096 lanes, a multiple of 256 (padded with lanes of the family itself); every family exists for fp32 and fp64
and for the packed and the scalar mode.  The conditions a family is built for are conditions on the reference alone: a
builder searches or rejects with the oracle's diagnostics (the normal against the ray, the front bit, the branch code).

The scene is one table for every family: random_spheres(100) (s100: hits on it come from oracle_nearest_hit) and,
after it, spheres that exist only to be named as a lane's hit: unit spheres at the origin of every material extreme,
the same with radius -1, and tiny, negative and huge radii elsewhere.  next_ray gathers the centre, the radius and the
material of hit_i and never asks whether the ray meets the sphere, so a lane may put its hit anywhere.  The material
table is stored in reverse, so materials[material[i]] is not materials[i]; sphere 0 (the ground) and the last sphere
are both hit.
"""
import functools
import zlib

import numpy as np

import independent_v2 as iv
import oracle_bind as ob
import rt_mi355x as rt

SEED = 0xDEADBEEF5EED0001   # a high word: the fp32 key fold is part of what is compared
DTYPES = {"f32": np.float32, "f64": np.float64}
MODES = ("packed", "scalar")
FAMILIES = ("ordinary", "front_bit", "tir", "schlick", "clamp", "near_zero", "colour", "scalar_normals", "camera",
            "mixed")
BLOCK, WAVE = 256, 64
IDLE, CAMERA, SCATTER = 0, 1, 2
CODE = {name: i for i, name in enumerate(ob.BRANCHES)}
NO_CODE = 255
LD = np.longdouble
UNTOUCHED = -12345.0     # what an idle lane's o, d and colour hold
FIELDS = ("role", "colx", "rowy", "pix", "sid", "k", "hit_i", "hit_t", "o", "d", "c")


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def prec_of(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


# ---------------------------------------------------------------- the scene
_SPECIALS = [
    # name, centre, radius, material
    ("lam_mid", (0, 0, 0), 1.0, rt.Lambertian((0.7, 0.5, 0.3))),
    ("lam_black", (0, 0, 0), 1.0, rt.Lambertian((0.0, 0.0, 0.0))),
    ("met_f1", (0, 0, 0), 1.0, rt.Metal((0.8, 0.8, 0.8), 1.0)),
    ("met_neg", (0, 0, 0), 1.0, rt.Metal((0.8, 0.6, 0.4), -0.5)),
    ("met_f0", (0, 0, 0), 1.0, rt.Metal((1.0, 1.0, 1.0), 0.0)),
    ("met_black", (0, 0, 0), 1.0, rt.Metal((0.0, 0.0, 0.0), 0.0)),
    ("g15", (0, 0, 0), 1.0, rt.Dielectric(1.5, False)),
    ("g15h", (0, 0, 0), 1.0, rt.Dielectric(1.5, True)),
    ("g24", (0, 0, 0), 1.0, rt.Dielectric(2.4, False)),
    ("g24h", (0, 0, 0), 1.0, rt.Dielectric(2.4, True)),
    ("g10003", (0, 0, 0), 1.0, rt.Dielectric(1.0003, False)),
    ("g1", (0, 0, 0), 1.0, rt.Dielectric(1.0, False)),
    ("g07", (0, 0, 0), 1.0, rt.Dielectric(0.7, False)),
    ("g1e-3", (0, 0, 0), 1.0, rt.Dielectric(1e-3, False)),
    ("g1e3", (0, 0, 0), 1.0, rt.Dielectric(1e3, False)),
    ("neg_lam", (0, 0, 0), -1.0, rt.Lambertian((1.0, 1.0, 1.0))),
    ("neg_met", (0, 0, 0), -1.0, rt.Metal((0.8, 0.8, 0.8), 1.0)),
    ("neg_g15", (0, 0, 0), -1.0, rt.Dielectric(1.5, False)),
    ("tiny_lam", (0.3, -0.2, 0.5), 1e-3, rt.Lambertian((0.7, 0.5, 0.3))),
    ("tiny_met", (0.3, -0.2, 0.5), 1e-3, rt.Metal((0.8, 0.6, 0.4), -0.5)),
    ("tiny_g15", (0.3, -0.2, 0.5), 1e-3, rt.Dielectric(1.5, False)),
    ("neg02_lam", (1.15, 0.2, 1.6), -0.2, rt.Lambertian((0.7, 0.5, 0.3))),
    ("neg02_g24", (1.15, 0.2, 1.6), -0.2, rt.Dielectric(2.4, False)),
    ("sky_lam", (0.0, 1000.5, 0.0), -1000.0, rt.Lambertian((0.7, 0.5, 0.3))),
    ("sky_g15h", (0.0, 1000.5, 0.0), -1000.0, rt.Dielectric(1.5, True)),
    ("lam_white", (0, 0, 0), 1.0, rt.Lambertian((1.0, 1.0, 1.0))),   # the last sphere
]
N_S100 = 100


@functools.lru_cache(maxsize=None)
def s100():
    return rt.scenes.random_spheres(N_S100).flatten()


@functools.lru_cache(maxsize=None)
def table():
    base = s100()
    mats = list(base.materials) + [s[3] for s in _SPECIALS]
    centre = np.vstack([base.center, np.array([s[1] for s in _SPECIALS], np.float64)])
    radius = np.concatenate([base.radius, [s[2] for s in _SPECIALS]])
    nm = len(mats)
    own = np.concatenate([base.material, len(base.materials) + np.arange(len(_SPECIALS))])
    return rt.FlatScene(centre, radius, (nm - 1 - own).astype(np.uint32), mats[::-1])


SP = {s[0]: N_S100 + i for i, s in enumerate(_SPECIALS)}
SP["ground"] = 0


def material_of(i):
    f = table()
    return f.materials[int(f.material[i])]


# ---------------------------------------------------------------- cameras
CAMERAS = {
    "main": lambda: rt.camera_new_py(16, 9, **rt.MAIN_CAMERA),
    "defocus": lambda: rt.camera_new_py(7, 5, **dict(rt.MAIN_CAMERA, defocus_angle=0.6)),
    "one": lambda: rt.camera_new_py(1, 1, **rt.MAIN_CAMERA),
    "minus_zero": lambda: rt.camera_new_py(8, 5, **dict(rt.MAIN_CAMERA, center=(16.0, 2.0, -0.0), look_at=(0.0, 0.0, -3.0))),
}


@functools.lru_cache(maxsize=None)
def camera(name):
    return CAMERAS[name]()


def host_pinhole(cam, dtype):
    """frame_params' pinhole flag: the defocus vectors are zero in T and the centre has no -0.0."""
    du, dv, ce = (np.array(list(v), np.float64).astype(dtype) for v in (cam.du, cam.dv, cam.center))
    return bool((du == 0).all() and (dv == 0).all() and not ((ce == 0) & np.signbit(ce)).any())


# ---------------------------------------------------------------- lanes
class Lanes:
    """n lanes: role u8; colx, rowy, pix, sid, k u32; hit_i i32; hit_t [n], o, d, c [3, n] in dtype."""

    def __init__(self, dtype, n):
        self.dtype, self.n = np.dtype(dtype).type, n
        self.role = np.zeros(n, np.uint8)
        self.colx, self.rowy, self.pix, self.sid, self.k = (np.zeros(n, np.uint32) for _ in range(5))
        self.hit_i = np.zeros(n, np.int32)
        self.hit_t = np.ones(n, dtype)
        self.o, self.d, self.c = (np.full((3, n), UNTOUCHED, dtype) for _ in range(3))

    def take(self, idx):
        idx = np.asarray(idx)
        out = Lanes(self.dtype, idx.size)
        for f in FIELDS:
            setattr(out, f, np.ascontiguousarray(getattr(self, f)[..., idx]))
        return out

    def copy(self):
        return self.take(np.arange(self.n))

    @staticmethod
    def cat(parts):
        out = Lanes(parts[0].dtype, sum(p.n for p in parts))
        for f in FIELDS:
            setattr(out, f, np.ascontiguousarray(np.concatenate([getattr(p, f) for p in parts], axis=-1)))
        return out

    def padded(self):
        """Padded to a multiple of 256 with the family's own first lanes."""
        m = -(-self.n // BLOCK) * BLOCK
        return self if m == self.n else self.take(np.arange(m) % self.n)

    def with_roles(self, keep):
        """The same launch with every lane of another role idle (its o, d, c as they are)."""
        out = self.copy()
        out.role[out.role != keep] = IDLE
        return out


def scatter_lanes(dtype, o, d, hit_i, hit_t, key=("key",), c=None, k=None, pix=None, sid=None):
    n = np.asarray(o).shape[1]
    la = Lanes(dtype, n)
    rng = _rng("lanes", *key, n)
    la.role[:] = SCATTER
    la.o, la.d = np.ascontiguousarray(o, dtype), np.ascontiguousarray(d, dtype)
    la.hit_i[:] = hit_i
    la.hit_t[:] = hit_t
    la.c = np.ascontiguousarray(rng.uniform(0.05, 1.0, (3, n)).astype(dtype) if c is None else c, dtype)
    # the counters' whole ranges: sid < 2^20, any pixel, bounce < 3839 (fp32's 257 + k < 2^12)
    la.k[:] = np.where(rng.random(n) < 0.9, rng.integers(0, 50, n), rng.integers(50, 3839, n)) if k is None else k
    la.pix[:] = np.where(rng.random(n) < 0.5, rng.integers(0, 1 << 20, n), rng.integers(0, 1 << 32, n)) if pix is None else pix
    la.sid[:] = np.where(rng.random(n) < 0.5, rng.integers(0, 64, n), rng.integers(0, 1 << 20, n)) if sid is None else sid
    if k is None and n >= 4:
        la.k[:2], la.sid[:2], la.pix[:2] = (0, 3838), (0, (1 << 20) - 1), (0, 0xFFFFFFFF)
    return la


class Launch:
    def __init__(self, name, cam_name, lanes, tags=None):
        assert lanes.n % BLOCK == 0 and 0 < lanes.n <= 4096, lanes.n
        self.name, self.cam_name, self.lanes = name, cam_name, lanes
        self.tags = tags or {}     # per-lane arrays of what the builder aimed at

    @property
    def cam(self):
        return camera(self.cam_name)


class Reference:
    """The oracle's result of a launch: o, d, c [3, n]; for scatter lanes nrm, front and the branch code (NO_CODE
    elsewhere)."""


def reference(la, mode, cam):
    ref = Reference()
    ref.o, ref.d, ref.c = la.o.copy(), la.d.copy(), la.c.copy()
    ref.nrm = np.zeros_like(la.o)
    ref.front = np.zeros(la.n, np.uint8)
    ref.code = np.full(la.n, NO_CODE, np.uint8)
    s = np.flatnonzero(la.role == SCATTER)
    if s.size:
        o, d, c, nrm, front, code = ob.oracle_next_ray(table(), SEED, mode, la.o[:, s], la.d[:, s], la.hit_i[s], la.hit_t[s],
                                                       la.sid[s], la.pix[s], la.k[s], la.c[:, s])
        ref.o[:, s], ref.d[:, s], ref.c[:, s], ref.nrm[:, s], ref.front[s], ref.code[s] = o, d, c, nrm, front, code
    m = np.flatnonzero(la.role == CAMERA)
    if m.size:
        o, d = ob.oracle_get_ray(la.dtype, cam, SEED, la.colx[m], la.rowy[m], la.pix[m], la.sid[m])
        ref.o[:, m], ref.d[:, m], ref.c[:, m] = o, d, 1.0
    return ref


def code_counts(code):
    return {name: int((code == i).sum()) for i, name in enumerate(ob.BRANCHES)}


# ---------------------------------------------------------------- geometry helpers (extended precision, then rounded)
def _unit(v):
    return v / np.sqrt((v * v).sum(0))


def _dirs(rng, n):
    return _unit(rng.standard_normal((3, n)).astype(LD))


def _perp(rng, nh):
    q = rng.standard_normal(nh.shape).astype(LD)
    return _unit(q - (q * nh).sum(0) * nh)


def _ulp_step(x, j):
    """x moved up by j (an int array) units in the last place; no step crosses zero."""
    s = np.int32 if x.dtype == np.float32 else np.int64
    b = x.view(s)
    out = np.where(b < 0, b - j.astype(s), b + j.astype(s)).astype(s)
    assert ((out < 0) == (b < 0)).all()
    return out.view(x.dtype)


def plain_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fused_dot(a, b):
    """PackedVec3::dot per lane, exactly (independent_v2's fma)."""
    T = iv.F32 if a.dtype == np.float32 else float
    return np.array([iv.pk_dot(tuple(T(x) for x in a[:, i]), tuple(T(x) for x in b[:, i])) for i in range(a.shape[1])], a.dtype)


def _hit_lanes(dtype, centre, radius, nh, dh, t, hit_i, key):
    """Lanes that hit the sphere (centre, |radius|) at centre + |radius| nh travelling along dh: o = p - dh t."""
    p = np.asarray(centre, LD)[:, None] + abs(radius) * nh
    d = dh.astype(dtype)
    tt = np.asarray(t, LD).astype(dtype)
    o = (p - d.astype(LD) * tt.astype(LD)).astype(dtype)
    return scatter_lanes(dtype, o, d, hit_i, tt, key)


def _geom(i):
    f = table()
    return f.center[i], f.radius[i]


# ---------------------------------------------------------------- a. ordinary
N_ORDINARY = 2048


@functools.lru_cache(maxsize=None)
def ordinary_lanes(prec, mode, n=N_ORDINARY, scaled_half=True):
    """Hits of oracle_nearest_hit on s100 (the lane's mode), aimed at every sphere and, for the branches glass takes,
    at the glass spheres from outside and from inside; the second half with |d|^2 log-uniform in [1e-6, 1e6]."""
    dtype = DTYPES[prec]
    rng = _rng("ordinary", prec, mode)
    base = s100()
    glass = np.array([i for i in range(N_S100) if isinstance(base.materials[base.material[i]], rt.Dielectric)])
    m = 6 * n
    target = np.where(rng.random(m) < 0.45, rng.choice(glass, m), rng.integers(0, N_S100, m))
    C, R = base.center[target].T.astype(LD), base.radius[target].astype(LD)
    inside = (rng.random(m) < 0.5) & np.isin(target, glass)
    aim = C + R * 0.98 * np.sqrt(rng.random(m)) * _dirs(rng, m)       # a point of the target
    org = np.where(inside, C + R * 0.9 * rng.random(m) * _dirs(rng, m),
                   np.array([[0.0], [1.5], [0.0]], LD) + np.array([[14.0], [2.5], [14.0]], LD) * rng.uniform(-1, 1, (3, m)))
    org[1] = np.where(inside, org[1], np.abs(org[1]) + 0.3)
    dh = _unit(aim - org)
    scale = np.ones(m, LD)
    if scaled_half:
        scale[m // 2:] = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), m - m // 2))
    o, d = org.astype(dtype), (dh * scale).astype(dtype)
    idx, t = ob.oracle_nearest_hit(base, mode, o, d)
    if mode == "packed":
        # under Q1 a ray that starts inside a sphere never hits it, so the packed mode's own hits are all front faces
        # and glass of ior 1.5 never refuses to refract; the ROOT2 kernels run the same next_ray<T, false> on back
        # faces, so the rays that start inside glass take their hits from that mode
        idx2, t2 = ob.oracle_nearest_hit(base, "root2", o, d)
        idx, t = np.where(inside, idx2, idx), np.where(inside, t2, t)
    keep = np.flatnonzero(idx >= 0)
    first, second = keep[keep < m // 2], keep[keep >= m // 2]
    la = None
    for attempt in range(1, 7):   # the same draw, more of it kept until every branch has its share
        sel = np.concatenate([first[:n // 2], second[:n - n // 2]])
        assert sel.size == n, (first.size, second.size)
        la = scatter_lanes(dtype, o[:, sel], d[:, sel], idx[sel], t[sel], ("ordinary", prec, mode))
        counts = code_counts(reference(la, mode, camera("main")).code)
        if all(v >= 32 for kname, v in counts.items() if kname != "near_zero"):
            return la
        first, second = np.roll(first, -n // 4), np.roll(second, -n // 4)
    raise AssertionError(f"ordinary/{prec}/{mode}: a branch has fewer than 32 lanes: {counts}")


def ordinary(prec, mode):
    return [Launch("ordinary", "main", ordinary_lanes(prec, mode))]


# ---------------------------------------------------------------- b. the front bit at dot == 0
FRONT_MATERIALS = ("lam_mid", "met_f1", "g15")
N_FRONT = 256    # geometries; each runs on the three materials


@functools.lru_cache(maxsize=None)
def front_bit(prec, mode):
    """A unit sphere at the origin and directions within 4 ulp of the tangent plane at the hit.  Of the N_FRONT
    geometries at least 64 have different front bits under the plain and the fused dot, at least 64 a plain dot of
    exactly +-0; the rest graze.  tags: plain, fused (the two dots against the reference's unflipped normal)."""
    dtype = DTYPES[prec]
    rng = _rng("front", prec, mode)
    m = 6000
    nh = _dirs(rng, m)
    th = _perp(rng, nh)
    eps = LD(np.finfo(dtype).eps)
    dh = th + nh * eps * rng.integers(-4, 5, m) * 0.5
    la = _hit_lanes(dtype, (0, 0, 0), 1.0, nh, dh, np.ones(m), SP["lam_mid"], ("front", prec, mode))
    ref = reference(la, mode, camera("main"))
    normal = ref.nrm * np.where(ref.front == 1, 1, -1).astype(dtype)     # the normal before the flip
    plain = plain_dot(la.d, normal)
    near = np.flatnonzero(np.abs(plain.astype(np.float64)) <= 8 * float(eps))
    fused = np.full(m, np.nan, dtype)
    fused[near] = fused_dot(la.d[:, near], normal[:, near])
    used = fused if mode == "packed" else plain
    assert np.array_equal((used[near] < 0), ref.front[near] == 1), "the reference's front bit is not the dot's sign"
    differ = near[(plain[near] < 0) != (fused[near] < 0)]
    zero = near[plain[near] == 0]
    assert differ.size >= 64 and zero.size >= 64, (differ.size, zero.size)
    rest = np.setdiff1d(near, np.concatenate([differ[:96], zero[:96]]))
    sel = np.concatenate([differ[:96], zero[:96], rest])[:N_FRONT]
    assert sel.size == N_FRONT
    parts, tags = [], {"plain": [], "fused": []}
    for name in FRONT_MATERIALS:
        part = la.take(sel)
        part.hit_i[:] = SP[name]
        parts.append(part)
        tags["plain"].append(plain[sel])
        tags["fused"].append(fused[sel])
    return [Launch("front_bit", "main", Lanes.cat(parts), {k: np.concatenate(v) for k, v in tags.items()})]


# ---------------------------------------------------------------- straddling pairs (c, d)
def straddle(prec, mode, nh, dh, hit_i, one, others, key, sid=None, pix=None, k=None, span=48, scan=False):
    """For each base (hit at nh on the unit sphere at the origin, direction dh): step the component of d that moves
    cos(theta) most by single ulps through [-span, span] and keep the first two neighbours of which one takes the
    branch `one` and the other a branch of `others`.  Returns (lanes: the pairs, lane 2j and 2j + 1 adjacent, their
    codes).  The root is the smallest valid one, 0.001: the hit point then hardly moves with the stepped direction (at
    t = 1 and nearly head-on, the scalar mode's unnormalised normal would move with it and cancel the step)."""
    dtype = DTYPES[prec]
    m = nh.shape[1]
    base = _hit_lanes(dtype, (0, 0, 0), 1.0, nh, dh, np.full(m, 0.001), hit_i, key)
    if sid is not None:
        base.sid[:], base.pix[:], base.k[:] = sid, pix, k
    comp = np.argmax(np.abs(nh.astype(np.float64)) * np.abs(base.d.astype(np.float64)), axis=0)
    steps = np.arange(-span, span + 1)
    rep = base.take(np.repeat(np.arange(m), steps.size))
    j = np.tile(steps, m)
    cc = np.repeat(comp, steps.size)
    col = np.arange(rep.n)
    rep.d[cc, col] = _ulp_step(rep.d[cc, col], j)
    code = reference(rep, mode, camera("main")).code.reshape(m, steps.size)
    a, b = code[:, :-1], code[:, 1:]
    flip = ((a == one) & np.isin(b, others)) | (np.isin(a, others) & (b == one))
    has = flip.any(1)
    at = flip.argmax(1)
    rows = np.flatnonzero(has)
    pick = np.stack([rows * steps.size + at[rows], rows * steps.size + at[rows] + 1], 1).ravel()
    if scan:
        return rep.take(pick), code.ravel()[pick], rep
    return rep.take(pick), code.ravel()[pick]


def _cone(nh, th, cos_t, outward):
    """Unit directions at angle acos(cos_t) from the hit's normal: leaving the sphere (a back-face hit) or entering."""
    sin_t = np.sqrt(1 - cos_t * cos_t)
    return (nh * cos_t if outward else -nh * cos_t) + th * sin_t


TIR_CASES = (("g15", True, 1.5), ("g24", True, 2.4), ("g10003", True, 1.0003), ("g07", False, 1 / 0.7), ("g1e-3", False, 1e3))
N_TIR_BASES = 40   # per case: up to 80 lanes each


@functools.lru_cache(maxsize=None)
def tir(prec, mode):
    """Back-face hits at the critical angle of ior 1.5, 2.4, 1.0003 and front-face hits of ior 0.7 and 1e-3: adjacent
    directions, one ulp apart in one component, on the two sides of ratio sin(theta) > 1."""
    rng = _rng("tir", prec, mode)
    parts, equal = [], []
    for name, outward, ratio in TIR_CASES:
        m = 6 * N_TIR_BASES
        nh = _dirs(rng, m)
        sin_c = LD(1) / LD(ratio)
        got, code, rep = straddle(prec, mode, nh, _cone(nh, _perp(rng, nh), np.sqrt(1 - sin_c * sin_c), outward), SP[name],
                                  CODE["cannot_refract"], (CODE["schlick_reflect"], CODE["refract"]), ("tir", prec, mode, name),
                                  scan=True)
        assert got.n >= 16, (name, prec, mode, got.n)
        parts.append(got.take(np.arange(min(got.n, 2 * N_TIR_BASES))))
        # ... and the scanned directions at which ratio sin(theta) is exactly 1: neither side of the comparison
        _, prod = sin_product(rep, reference(rep, mode, camera("main")))
        equal.append(rep.take(np.flatnonzero(prod == 1)[:8]))
    pairs, equal = Lanes.cat(parts), Lanes.cat(equal)
    la = Lanes.cat([pairs, equal])
    return [Launch("tir", "main", la.padded(), {"n": la.n, "pairs": pairs.n, "equal": equal.n})]


SCHLICK_CASES = (("g24", False), ("g07", True))    # front face: r0_front of 2.4; back face: r0_back of 0.7
N_SCHLICK = 48   # pairs per case


@functools.lru_cache(maxsize=None)
def schlick(prec, mode):
    """For a lane's own draw ua: cos(theta) solved from r0 + (1 - r0)(1 - cos)^5 = ua, then adjacent directions on the
    two sides of reflectance > ua.  Front-face hits of ior 2.4 and back-face hits of ior 0.7: neither can refuse to
    refract (ratio < 1), and each reads another member of the host's (r0_front, r0_back) pair."""
    dtype = DTYPES[prec]
    rng = _rng("schlick", prec, mode)
    parts = []
    for name, outward in SCHLICK_CASES:
        ior = LD(material_of(SP[name]).index_of_refraction)
        ratio = ior if outward else 1 / ior
        r0 = ((1 - ratio) / (1 + ratio)) ** 2
        m = 8 * N_SCHLICK
        sid, pix, k = rng.integers(0, 1 << 20, m), rng.integers(0, 1 << 32, m), rng.integers(0, 3839, m)
        _, ua, _ = ob.oracle_draw(dtype, sid, pix, k, np.full(m, 2), SEED)
        ok = (ua.astype(LD) > r0 + LD(0.02)) & (ua < 0.98)
        sid, pix, k, ua = sid[ok], pix[ok], k[ok], ua[ok].astype(LD)
        cos_t = 1 - ((ua - r0) / (1 - r0)) ** LD(0.2)
        nh = _dirs(rng, cos_t.size)
        la, code = straddle(prec, mode, nh, _cone(nh, _perp(rng, nh), cos_t, outward), SP[name],
                            CODE["schlick_reflect"], (CODE["refract"],), ("schlick", prec, mode, name), sid, pix, k)
        assert la.n >= 2 * 32, (name, prec, mode, la.n)
        parts.append(la.take(np.arange(min(la.n, 2 * N_SCHLICK))))
    la = Lanes.cat(parts)
    return [Launch("schlick", "main", la.padded(), {"n": la.n})]


# ---------------------------------------------------------------- e. the clamp and sqrt_nd's contract
CLAMP_MATERIALS = ("g15", "g15h", "g24h", "g1")


def _lengths(dtype):
    one = dtype(1)
    return [one, np.nextafter(one, dtype(0)), np.nextafter(one, dtype(2)), dtype(2), dtype(1e3)]


@functools.lru_cache(maxsize=None)
def clamp(prec, mode):
    """Head-on hits, from outside and from inside, |d| = 1, 1 -+ 1 ulp, 2, 1e3, along the axes (the normal is exact:
    cos = |d| exactly, clamped from above; -|d| through the hollow flip, where 1 - cos^2 < 0 and sin is NaN) and along
    random normals (cos within ulps of those)."""
    dtype = DTYPES[prec]
    rng = _rng("clamp", prec, mode)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).T.astype(LD)
    nh = np.concatenate([axes, _dirs(rng, 10)], axis=1)
    parts = []
    for name in CLAMP_MATERIALS:
        for s in _lengths(dtype):
            for outward in (False, True):
                dh = nh * LD(s) * (1 if outward else -1)
                parts.append(_hit_lanes(dtype, (0, 0, 0), 1.0, nh, dh, np.ones(nh.shape[1]), SP[name],
                                        ("clamp", prec, mode, name, float(s), outward)))
    la = Lanes.cat(parts)
    return [Launch("clamp", "main", la.padded(), {"n": la.n})]


def cos_theta(la, ref):
    """Material::get_hit_result's dot(-d, n) of dielectric lanes before its clamp to 1, from the reference's normal
    (NaN elsewhere), in the lanes' precision."""
    f = table()
    kinds = np.array([m.kind for m in f.materials])[f.material[la.hit_i]]
    hollow = np.array([getattr(m, "hollow", False) for m in f.materials])[f.material[la.hit_i]]
    raw = plain_dot(-la.d, ref.nrm * np.where(hollow, -1, 1).astype(la.dtype))
    return np.where((la.role == SCATTER) & (kinds == rt.Dielectric.kind), raw, np.nan).astype(la.dtype)


def sin_product(la, ref):
    """(1 - cos^2, ratio * sin(theta)) of dielectric lanes as get_hit_result computes them."""
    f = table()
    ior = np.array([getattr(m, "index_of_refraction", np.nan) for m in f.materials])[f.material[la.hit_i]].astype(la.dtype)
    with np.errstate(all="ignore"):
        ct = np.minimum(cos_theta(la, ref), la.dtype(1))
        arg = la.dtype(1) - ct * ct
        ratio = np.where(ref.front == 1, la.dtype(1) / ior, ior)
        return arg, ratio * np.sqrt(arg)


# ---------------------------------------------------------------- f. near zero
N_NEAR = 384


@functools.lru_cache(maxsize=None)
def near_zero(prec, mode):
    """Lambertian hits at the origin's unit sphere with o = -2 rv, d = rv, t = 1, rv the lane's own random unit vector:
    the hit is -rv exactly, and where the normal's length rounds to 1 (always under scalar: radius 1 and -1) the sum
    rv + n is exactly zero.  Then lanes with o moved along rv's smallest component, so that this component of rv + n
    lies on either side of 1e-8 (tags: perturbed, and the sum's largest magnitude)."""
    dtype = DTYPES[prec]
    rng = _rng("near", prec, mode)
    m = N_NEAR
    sid, pix, k = rng.integers(0, 1 << 20, m), rng.integers(0, 1 << 32, m), rng.integers(0, 3839, m)
    _, ua, ub = ob.oracle_draw(dtype, sid, pix, k, np.full(m, 2), SEED)
    rv = ob.oracle_unit_vec(ua, ub)
    hit = np.where(np.arange(m) % 2 == 0, SP["lam_white"], SP["neg_lam"] if mode == "scalar" else SP["lam_mid"])
    exact = scatter_lanes(dtype, dtype(-2) * rv, rv, hit, np.ones(m), ("near", prec, mode), k=k, pix=pix, sid=sid)
    # perturbed: the smallest component e of rv, below 2^-4 (fp32: its ulp is then below 4e-9)
    e = np.argmin(np.abs(rv), axis=0)
    small = np.flatnonzero(np.abs(rv[e, np.arange(m)]) < 0.0625)
    rel = np.tile(np.array([-0.7, -0.4, -0.1, -1e-3, -1e-6, 1e-6, 1e-3, 0.1, 0.5, 2.0, 5.0]), small.size)[:small.size * 11]
    rows = np.repeat(small, 11)
    pert = exact.take(rows)
    delta = (LD(1e-8) * (1 + rel.astype(LD))).astype(dtype)
    ee = e[rows]
    col = np.arange(rows.size)
    pert.o[ee, col] = pert.o[ee, col] + delta * np.where(rng.random(rows.size) < 0.5, 1, -1).astype(dtype)
    la = Lanes.cat([exact, pert])
    la = la.take(np.arange(min(la.n, 4096)))
    perturbed = np.arange(la.n) >= m
    return [Launch("near_zero", "main", la.padded(), {"n": la.n, "perturbed": perturbed})]


# ---------------------------------------------------------------- g. colour
def _colours(dtype):
    fi = np.finfo(dtype)
    tiny, sub = dtype(fi.tiny), dtype(fi.smallest_subnormal)
    return np.array([0.0, -0.0, sub, dtype(3) * sub, tiny * dtype(0.25), tiny, tiny * dtype(1.5), tiny * dtype(2.5), 1.0, 0.5,
                     fi.max, 1e-20, 0.999], dtype)


COLOUR_MATERIALS = ("lam_white", "lam_black", "lam_mid", "met_f0", "met_f1", "met_neg", "met_black", "g15", "g24h")


@functools.lru_cache(maxsize=None)
def colour(prec, mode):
    """Colours of 0, -0, subnormals and normals whose product with an albedo of 0.7, 0.5 or 0.3 is subnormal or rounds
    to 0, on albedos 0 and 1, fuzz 0, 1 and -0.5, and on glass, which must hand the colour back bit for bit."""
    dtype = DTYPES[prec]
    rng = _rng("colour", prec, mode)
    vals = _colours(dtype)
    parts = []
    for name in COLOUR_MATERIALS:
        m = 3 * vals.size
        nh = _dirs(rng, m)
        dh = _unit(-nh * rng.uniform(0.2, 1.0, m) + _perp(rng, nh) * rng.uniform(0.0, 1.0, m))
        part = _hit_lanes(dtype, (0, 0, 0), 1.0, nh, dh, rng.uniform(0.5, 2.0, m), SP[name], ("colour", prec, mode, name))
        for ch in range(3):
            part.c[ch] = np.roll(np.repeat(vals, 3), ch * 5)
        parts.append(part)
    la = Lanes.cat(parts)
    return [Launch("colour", "main", la.padded(), {"n": la.n})]


# ---------------------------------------------------------------- h. scalar normals
RADII_SPHERES = ("ground", "tiny_lam", "tiny_met", "tiny_g15", "neg02_lam", "neg02_g24", "neg_lam", "neg_met", "neg_g15",
                 "sky_lam", "sky_g15h")
N_RADII = 24    # per sphere and side


@functools.lru_cache(maxsize=None)
def scalar_normals(prec, mode):
    """Hits on radii 1000, 1e-3, -0.2, -1 and -1000, from both sides: (p - c) / radius has a length that differs from
    1 by rounding and, for a negative radius, the opposite sign.  Interleaved with ordinary lanes half and half in
    every wave (dvs ballots).  tags: special, the lanes of this family's own."""
    dtype = DTYPES[prec]
    rng = _rng("radii", prec, mode)
    parts = []
    for name in RADII_SPHERES:
        c, r = _geom(SP[name])
        for outward in (False, True):
            nh = _dirs(rng, N_RADII)
            if name == "ground":
                nh[1] = np.abs(nh[1]) * 50 + 1      # near the top: where the scene's rays meet the ground
                nh = _unit(nh)
            if name.startswith("sky"):
                nh[1] = -np.abs(nh[1]) * 50 - 1
                nh = _unit(nh)
            dh = _unit(nh * (1 if outward else -1) * rng.uniform(0.05, 1.0, N_RADII) + _perp(rng, nh) * rng.uniform(0, 1, N_RADII))
            parts.append(_hit_lanes(dtype, c, r, nh, dh, rng.uniform(0.5, 3.0, N_RADII) * min(1.0, abs(r) * 100), SP[name],
                                    ("radii", prec, mode, name, outward)))
    own = Lanes.cat(parts)
    n = -(-own.n // 128) * 128
    own = own.take(np.arange(n) % own.n)
    fill = ordinary_lanes(prec, mode).take(np.arange(n))
    both = Lanes.cat([own, fill])
    order = np.arange(2 * n).reshape(2, n // 32, 32).transpose(1, 0, 2).ravel()    # 32 own, 32 ordinary, ...
    special = order < n
    return [Launch("scalar_normals", "main", both.take(order), {"special": special})]


# ---------------------------------------------------------------- i. camera lanes
def camera_lanes(dtype, cam, n_sid=16):
    W, H = cam.image_width, cam.image_height
    pix = np.repeat(np.arange(W * H), n_sid)
    la = Lanes(dtype, pix.size)
    la.role[:] = CAMERA
    la.pix[:], la.colx[:], la.rowy[:] = pix, pix % W, pix // W
    la.sid[:] = np.tile(np.arange(n_sid), W * H)
    return la


@functools.lru_cache(maxsize=None)
def camera_family(prec, mode):
    """Every pixel, samples 0 .. 15: the main pinhole camera at 16 x 9; the same with a defocus disk at 7 x 5 (the
    rejection loop diverges); a 1 x 1 frame; a pinhole camera whose centre has a -0.0 (the host's flag is then off)."""
    dtype = DTYPES[prec]
    return [Launch(f"camera:{name}", name, camera_lanes(dtype, camera(name)).padded()) for name in CAMERAS]


# ---------------------------------------------------------------- j. mixed waves
def _tiny_lane(dtype):
    """A scatter lane whose |hit - centre|^2 is tiny (1e-36: below sqrt_len's 2^-96) and not zero."""
    o = np.array([[1e-18], [0.0], [0.0]], dtype)
    return scatter_lanes(dtype, o, o * dtype(0.5), SP["lam_mid"], np.zeros(1), ("tiny",), k=[3], pix=[5], sid=[7])


@functools.lru_cache(maxsize=None)
def mixed(prec, mode):
    """Scatter lanes of (a) and camera lanes of (i, the main camera) in one wave: all scatter, all camera, alternating,
    one camera lane among 63 scatter, one scatter lane among 63 camera, four waves each; then the same with 32 lanes
    of every wave idle.  Second launch: ordinary lanes with lane 7 of every odd wave replaced by a lane whose
    |vec|^2 is tiny, so that the others' sqrt_len takes its other path."""
    dtype = DTYPES[prec]
    sc = ordinary_lanes(prec, mode)
    cm = camera_lanes(dtype, camera("main"))
    lane = np.arange(WAVE)
    patterns = [np.zeros(WAVE, bool), np.ones(WAVE, bool), lane % 2 == 1, lane == 21, lane != 40]   # True: camera
    parts, si, ci = [], 0, 0
    for idle in (False, True):
        for pat in patterns:
            for w in range(4):
                a, b = sc.take(np.arange(si, si + WAVE) % sc.n), cm.take(np.arange(ci, ci + WAVE) % cm.n)
                si, ci = si + WAVE, ci + 37 * WAVE
                wave = Lanes.cat([a, b]).take(np.where(pat, WAVE + lane, lane))
                if idle:
                    off = (lane + w) % 2 == 0 if w < 2 else (lane < 32) == (w == 2)
                    wave.role[off] = IDLE
                    for f in ("o", "d", "c"):
                        getattr(wave, f)[:, off] = UNTOUCHED
                parts.append(wave)
    la = Lanes.cat(parts)
    broken = sc.take(np.arange(1024, 1024 + 512))
    t = _tiny_lane(dtype)
    for w in range(1, 8, 2):
        for f in FIELDS:
            getattr(broken, f)[..., w * WAVE + 7] = getattr(t, f)[..., 0]
    tiny = np.zeros(broken.n, bool)
    tiny[np.arange(1, 8, 2) * WAVE + 7] = True
    return [Launch("mixed:roles", "main", la), Launch("mixed:lane7", "main", broken, {"tiny": tiny})]


BUILDERS = {"ordinary": ordinary, "front_bit": front_bit, "tir": tir, "schlick": schlick, "clamp": clamp,
            "near_zero": near_zero, "colour": colour, "scalar_normals": scalar_normals, "camera": camera_family,
            "mixed": mixed}


def family(name, prec, mode):
    return BUILDERS[name](prec, mode)


@functools.lru_cache(maxsize=None)
def family_reference(name, prec, mode):
    return [reference(ln.lanes, mode, ln.cam) for ln in family(name, prec, mode)]


# ---------------------------------------------------------------- the second reference, per lane, with mutations
MUTANTS = ("plain_front", "cannot_ge", "schlick_ub", "r0_swapped", "no_hollow", "near_1e-7", "near_1e-9", "unflipped",
           "abs_radius")


def _materials_py(prec):
    T = iv.F32 if prec == "f32" else float
    f = table()
    out = []
    for m in f.materials:
        a = m.to_abi()
        out.append(iv.Material(a.kind, tuple(a.albedo), a.fuzz, a.ior, a.hollow, prec))
        out[-1].fuzz = T(a.fuzz)    # the table's fuzz is already Metal::new's (negative values stay)
    return out


@functools.lru_cache(maxsize=None)
def scene_py(prec):
    T = iv.F32 if prec == "f32" else float
    f = table()
    cen = [tuple(T(x) for x in c) for c in f.center]
    return cen, [T(r) for r in f.radius], [int(x) for x in f.material], _materials_py(prec)


def _scatter_mutated(mat, d, normal, front, u1, u2, mutate):
    """Material::get_hit_result (materials.rs:54-147) from independent_v2's primitives, with one thing changed."""
    one = u1 * 0 + 1
    if mat.kind == 0:
        sd = iv.v_add(iv.random_unit_vector(u1, u2), normal)
        e = {"near_1e-7": 1e-7, "near_1e-9": 1e-9}.get(mutate, 1e-8)
        if abs(sd[0]) < e and abs(sd[1]) < e and abs(sd[2]) < e:
            sd = normal
        return mat.albedo, sd
    if mat.kind == 1:
        return mat.albedo, iv.v_add(iv.reflect(d, normal), iv.v_mul(iv.random_unit_vector(u1, u2), mat.fuzz))
    ratio = 1.0 / mat.ior if front else mat.ior
    n = iv.v_neg(normal) if (mat.hollow and mutate != "no_hollow") else normal
    cos_theta = iv.fmin(iv.v_dot(iv.v_neg(d), n), 1.0)
    sin_theta = iv.sqrt(1.0 - cos_theta * cos_theta)
    cannot = ratio * sin_theta >= 1.0 if mutate == "cannot_ge" else ratio * sin_theta > 1.0
    refl = True
    if not cannot:
        rr = (mat.ior if front else 1.0 / mat.ior) if mutate == "r0_swapped" else ratio
        q = (1.0 - rr) / (1.0 + rr)
        r0 = q * q
        m = 1.0 - cos_theta
        refl = r0 + (1.0 - r0) * (m * ((m * m) * (m * m))) > (u2 if mutate == "schlick_ub" else u1)
    return (one, one, one), (iv.reflect(d, n) if refl else iv.refract(d, n, ratio))


def next_ray_py(la, i, mode, cam_py, mutate=None):
    """Lane i of la by the second reference: (o, d, c) as tuples of scalars in the lane's precision."""
    prec = prec_of(la.dtype)
    T = iv.F32 if prec == "f32" else float
    if la.role[i] == IDLE:
        return tuple(T(x) for x in la.o[:, i]), tuple(T(x) for x in la.d[:, i]), tuple(T(x) for x in la.c[:, i])
    if la.role[i] == CAMERA:
        o, d = iv.get_ray(cam_py, int(la.colx[i]), int(la.rowy[i]), int(la.sid[i]), int(la.pix[i]), SEED, prec)
        return o, d, (T(1.0), T(1.0), T(1.0))
    cen, rad, smat, mats = scene_py(prec)
    h = int(la.hit_i[i])
    o, d, c = (tuple(T(x) for x in getattr(la, f)[:, i]) for f in ("o", "d", "c"))
    t = T(la.hit_t[i])
    loc = iv.v_add(o, iv.v_mul(d, t))                      # at_t
    vec = iv.v_sub(loc, cen[h])
    if mode == "scalar":
        r = abs(rad[h]) if mutate == "abs_radius" else rad[h]
        n = iv.v_div(vec, r)                               # objects.rs:242
        front = iv.v_dot(d, n) < 0.0                       # objects.rs:69-73
    else:
        n = iv.v_div(vec, iv.sqrt(iv.pk_len2(vec)))        # finalize, objects.rs:158
        front = (iv.v_dot(d, n) if mutate == "plain_front" else iv.pk_dot(d, n)) < 0.0
    if not front and mutate != "unflipped":
        n = iv.v_neg(n)
    u1, u2 = iv.uniforms(int(la.sid[i]), int(la.pix[i]), int(la.k[i]), 2, SEED, prec)
    mat = mats[smat[h]]
    if mutate is None:
        att, nd = iv.get_hit_result(mat, d, loc, n, front, u1, u2)
    else:
        att, nd = _scatter_mutated(mat, d, n, front, u1, u2, mutate)
    return loc, nd, (c[0] * att[0], c[1] * att[1], c[2] * att[2])


def camera_py(cam, prec):
    d = {"W": cam.image_width, "H": cam.image_height}
    for kname in ("center", "ulc", "vu", "vv", "du", "dv"):
        d[kname] = tuple(float(x) for x in getattr(cam, kname))
    return iv.camera_in(d, prec)


def lanes_py(la, idx, mode, cam, mutate=None):
    """(o, d, c) [3, len(idx)] of the listed lanes by the second reference."""
    cam_py = camera_py(cam, prec_of(la.dtype))
    out = [np.empty((3, len(idx)), la.dtype) for _ in range(3)]
    with np.errstate(all="ignore"):
        for j, i in enumerate(idx):
            for arr, v in zip(out, next_ray_py(la, int(i), mode, cam_py, mutate)):
                arr[:, j] = v
    return out
