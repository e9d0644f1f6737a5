"""Inputs and plain references of the device-math tests (tests/test_gpu_device_math.py runs them on the GPU,
tests/test_device_math_refs.py checks on the CPU that they are what they claim).

References are plain IEEE arithmetic in numpy: float32 / float64 element-wise operations, one rounding each,
no contraction.  Outputs are compared as bit patterns (same_bits); where the reference is NaN the other
side must be NaN, the payload is not compared.
"""
import math

import numpy as np

WAVE = 64
U32 = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


# ---------------------------------------------------------------- comparison
def same_bits(got, ref):
    """Element-wise: identical bit patterns, or both NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    if got.dtype.kind != "f":
        return got == ref
    u = U32[got.dtype]
    return (got.view(u) == ref.view(u)) | (np.isnan(got) & np.isnan(ref))


def assert_bits(got, ref, what, inputs=()):
    ok = same_bits(got, ref)
    if not ok.all():
        bad = np.argwhere(~ok)[:4]
        rows = []
        for b in bad:
            b = tuple(b)
            rows.append((b, got[b].tobytes().hex(), ref[b].tobytes().hex(), [np.asarray(x)[..., b[-1]].tolist() for x in inputs]))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ; (index, got, want, inputs): {rows}")


# ---------------------------------------------------------------- references
def ref_div(a, s):
    with np.errstate(all="ignore"):
        return a / s


def ref_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(x)


def ref_div_via_f64(a, s):
    """fp32 a / s as the float64 quotient rounded to float32 (53 >= 2 * 24 + 2: the double rounding is harmless)."""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) / s.astype(np.float64)).astype(np.float32)


def ref_sqrt_via_f64(x):
    with np.errstate(all="ignore"):
        return np.sqrt(x.astype(np.float64)).astype(np.float32)


def ref_unit(v):
    """geometry.rs:118-120: v / sqrt((x*x + y*y) + z*z)."""
    with np.errstate(all="ignore"):
        l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        return v / np.sqrt(l2)


def ref_len2(v):
    with np.errstate(all="ignore"):
        return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def ref_q8(v):
    """color.rs:54-64: sqrt, * 255.999, saturating `as u8` (NaN -> 0)."""
    T = v.dtype.type
    with np.errstate(all="ignore"):
        x = np.sqrt(v) * T(255.999)
        out = np.where(x >= T(255.0), T(255.0), np.trunc(np.where(x > T(0.0), x, T(0.0))))
    return out.astype(np.uint8)


def ref_div_dim(x, W):
    return x / x.dtype.type(W)


def host_rW(W):
    """rt_kernel.hip: RN(1/W) for W < 2^20, else 0 (plain division)."""
    return 1.0 / float(W) if W < (1 << 20) else 0.0


def ref_hit(hb, disc, idx, cnt, a, mode):
    """The plain rule over each lane's first cnt candidates (hb, disc, idx: [8, n]).
    packed: Sphere::hit_packed's first root (objects.rs:270-272) + PackedHitRecords::update (:140-155: nearer, or
    equal and a later sphere); root2: the second root when the first is invalid; scalar: Sphere::hit's roots
    (/ a) and Scene::hit's first minimum.  Returns (t, index), (+inf, -1) for no hit."""
    T = hb.dtype.type
    n = hb.shape[1]
    bt, bi = np.full(n, np.inf, hb.dtype), np.full(n, -1, np.int64)
    t001, inf = T(0.001), T(np.inf)
    with np.errstate(all="ignore"):
        inv_a = T(1.0) / a
        for c in range(hb.shape[0]):
            sd = np.sqrt(disc[c])
            if mode == "scalar":
                r1, r2 = (-hb[c] - sd) / a, (-hb[c] + sd) / a
            else:
                r1, r2 = (-hb[c] - sd) * inv_a, (-hb[c] + sd) * inv_a
            v1 = (r1 >= t001) & (r1 < inf)
            if mode == "packed":
                root, valid = r1, v1
            else:
                root, valid = np.where(v1, r1, r2), v1 | ((r2 >= t001) & (r2 < inf))
            i = idx[c].astype(np.int64)
            tie = (i < bi) if mode == "scalar" else (i > bi)
            take = (c < cnt) & valid & ((root < bt) | ((root == bt) & tie))
            bt, bi = np.where(take, root, bt), np.where(take, i, bi)
    return bt, bi.astype(np.int32)


# ---------------------------------------------------------------- contracts (rt_device.hpp)
def dvs_in_contract(v, s):
    """dvs's fast-path condition per lane: 2^-20 <= s <= 2^20 and every |a_i| >= 2^-100."""
    T = v.dtype.type
    return (s >= T(2.0 ** -20)) & (s <= T(2.0 ** 20)) & (np.abs(v).min(axis=0) >= T(2.0 ** -100))


def sqrt_len_in_contract(x):
    """sqrt_len's fast-path condition per lane.  fp32: no tiny nonzero argument of either sign; fp64: 2^-100 <= x <= 2^100."""
    if x.dtype == np.float32:
        return ~((x != 0) & (np.abs(x) < np.float32(2.0 ** -96)))
    return (x >= 2.0 ** -100) & (x <= 2.0 ** 100)


def sqrt_nd_in_contract(x):
    """fp32 sqrt_nd: +-0, >= 2^-96, +inf, <= -2^-96 or NaN."""
    return ~((x != 0) & (np.abs(x) < np.float32(2.0 ** -96)))


def waves_all(ok):
    """Per wave of 64 lanes: every lane ok (ok's length a multiple of 64)."""
    return ok.reshape(-1, WAVE).all(axis=1)


def break_lane7(a, value):
    """Run B of the mixed-wave tests: lane 7 of every odd wave replaced (last axis), a copy."""
    b = np.array(a, copy=True)
    b[..., WAVE + 7::2 * WAVE] = value
    return b


def broken_lanes(n):
    m = np.zeros(n, bool)
    m[WAVE + 7::2 * WAVE] = True
    return m


# ---------------------------------------------------------------- fp32 division next to a rounding boundary
def div_boundary_f32(r):
    """Every odd 24-bit S with M = r * S^-1 mod 2^25 >= 2^24 and X = (S*M - r) / 2^25 in [2^23, 2^24):
    X / S = M / 2^25 - r / (S * 2^25), within ~2^-48 relative of the float midpoint M / 2^25 (M is odd), on the
    side the sign of r says.  Returns uint64 arrays (X, S, M)."""
    S = np.arange((1 << 23) + 1, 1 << 24, 2, dtype=np.uint64)
    mask = np.uint64((1 << 25) - 1)
    inv = S.copy()                                    # S * S == 1 mod 8
    for _ in range(4):                                # Newton: 3 -> 6 -> 12 -> 24 -> 48 bits
        inv = (inv * (np.uint64(2) - S * inv)) & mask
    M = (np.uint64(r % (1 << 25)) * inv) & mask
    num = (S * M).astype(np.int64) - np.int64(r)      # S * M < 2^49
    X = (num >> np.int64(25)).astype(np.uint64)
    keep = (M >= np.uint64(1 << 24)) & (X >= np.uint64(1 << 23)) & (X < np.uint64(1 << 24))
    return X[keep], S[keep], M[keep]


DIV_R = (1, -1, 3, -3)


def div_boundary_f32_all():
    """The four r families, concatenated: (X, S, M, r) arrays."""
    parts = [div_boundary_f32(r) + (r,) for r in DIV_R]
    X, S, M = (np.concatenate([p[j] for p in parts]) for j in range(3))
    R = np.concatenate([np.full(p[0].size, p[3], np.int64) for p in parts])
    return X, S, M, R


# (exponent of s, exponents of the three numerators): s = S' 2^es and a_j = +-X' 2^ej with S', X' in [1, 2).
# Every a_j <= s in magnitude (unit()'s situation); the smallest component sits at 2^-100 or at ordinary magnitudes.
DIV_PLACEMENTS_F32 = ((-20, (-100, -21, -30)), (0, (0, -1, -100)), (19, (19, 0, -100)), (0, (0, -3, -7)), (19, (18, -100, 3)))


def place_f32(X, S, es, ea):
    s = np.ldexp(S.astype(np.float32), np.int32(es - 23))
    sign = (1.0, -1.0, 1.0)
    v = np.stack([np.ldexp(X.astype(np.float32) * np.float32(sg), np.int32(e - 23)) for e, sg in zip(ea, sign)])
    return v, s


def predicted_quotient_f32(M, R, es, ea):
    """The correctly rounded X 2^e / (S 2^es) by construction: the midpoint's neighbour on r's side."""
    q = (M.astype(np.int64) - np.sign(R)).astype(np.float32)     # even, < 2^25: exact in float32
    sign = (1.0, -1.0, 1.0)
    return np.stack([np.ldexp(q * np.float32(sg), np.int32(e - es - 25)) for e, sg in zip(ea, sign)])


# ---------------------------------------------------------------- fp64 division / sqrt next to a rounding boundary
def div_boundary_f64(count, seed):
    """The same construction with 53-bit S and Python integers: lists X, S, M, r (count cases)."""
    rnd = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        for s in rnd.integers(1 << 51, 1 << 52, 4096, dtype=np.int64):
            S = (int(s) << 1) | 1                                  # odd, in [2^52, 2^53)
            inv = pow(S, -1, 1 << 54)
            for r in DIV_R:
                M = (r * inv) % (1 << 54)
                X = (S * M - r) >> 54
                if M >= (1 << 53) and (1 << 52) <= X < (1 << 53):
                    assert X * (1 << 54) + r == S * M
                    out.append((X, S, M, r))
    out = out[:count]
    return tuple(np.array([o[j] for o in out], dtype=np.int64) for j in range(4))


DIV_PLACEMENTS_F64 = ((-20, (-100, -21, -30)), (0, (0, -1, -100)), (19, (19, 0, -100)), (0, (0, -3, -7)))


def place_f64(X, S, es, ea):
    s = np.ldexp(S.astype(np.float64), es - 52)
    sign = (1.0, -1.0, 1.0)
    v = np.stack([np.ldexp(X.astype(np.float64) * sg, e - 52) for e, sg in zip(ea, sign)])
    return v, s


def predicted_quotient_f64(M, R, es, ea):
    q = ((M - np.sign(R)) >> 1).astype(np.float64)                 # (M -+ 1) / 2 < 2^53: exact
    sign = (1.0, -1.0, 1.0)
    return np.stack([np.ldexp(q * sg, e - es - 53) for e, sg in zip(ea, sign)])


def sqrt_boundary_f64(count, seed):
    """Both 53-bit neighbours of M^2 for odd 54-bit M, scaled by 2^-106 into [1, 4): sqrt(x) lies within about
    2^-54 relative of M / 2^53... the midpoint of two doubles.  Returns (x float64 [2*count], exact roots)."""
    rnd = np.random.default_rng(seed)
    xs, roots = [], []
    for m in rnd.integers(1 << 52, 1 << 53, count, dtype=np.int64):
        M = (int(m) << 1) | 1
        sq = M * M
        sh = sq.bit_length() - 53
        for top in (sq >> sh, (sq >> sh) + 1):
            if top >= (1 << 53):
                continue
            xs.append(math.ldexp(float(top), sh - 106))
            roots.append(exact_sqrt_f64(top, sh - 106))
    return np.array(xs, np.float64), np.array(roots, np.float64)


def exact_sqrt_f64(m, e):
    """The double nearest to sqrt(m * 2^e) (m a positive int), by integer square root: ties cannot occur."""
    if e & 1:
        m, e = m << 1, e - 1
    sh = max(0, 110 - m.bit_length())
    sh += sh & 1
    r = math.isqrt(m << sh)                                        # >= 2^54: more than 53 bits
    extra = r.bit_length() - 53
    q, rem = r >> extra, r & ((1 << extra) - 1)
    half = 1 << (extra - 1)
    # sqrt is irrational or exact; r = floor: the fraction beyond `rem` only matters when rem == half - ... never a tie
    if rem >= half:
        q += 1
    return math.ldexp(float(q), (e - sh) // 2 + extra)


# ---------------------------------------------------------------- random arguments
def random_binades(dtype, n, lo, hi, seed, signed=False):
    """n values with uniform random significands and exponents uniform in [lo, hi)."""
    rnd = np.random.default_rng(seed)
    m = (1.0 + rnd.random(n)).astype(dtype)
    x = np.ldexp(m, rnd.integers(lo, hi, n).astype(np.int32))
    if signed:
        x = np.where(rnd.random(n) < 0.5, -x, x)
    return x.astype(dtype)


def random_vectors(dtype, n, lo, hi, seed):
    """[3, n]: one exponent per vector in [lo, hi], components in (-1, 1) times it."""
    rnd = np.random.default_rng(seed)
    c = rnd.uniform(-1.0, 1.0, (3, n)).astype(dtype)
    return np.ldexp(c, rnd.integers(lo, hi + 1, n).astype(np.int32)).astype(dtype)


def needle_vectors(dtype, n, seed):
    """One dominant axis (the needle rays of edge_scenes.py): the other two 2^-8 .. 2^-40 of it."""
    rnd = np.random.default_rng(seed)
    v = np.ldexp(rnd.uniform(-1.0, 1.0, (3, n)), -rnd.integers(8, 41, (3, n)))
    ax = rnd.integers(0, 3, n)
    v[ax, np.arange(n)] = rnd.uniform(0.5, 2.0, n) * rnd.choice([-1.0, 1.0], n)
    return np.ldexp(v, rnd.integers(-10, 11, n)).astype(dtype)


# ---------------------------------------------------------------- hit_update
def special_roots(dtype):
    T = np.dtype(dtype).type
    t001 = T(0.001)
    tiny = np.finfo(dtype).smallest_subnormal
    return np.array([0.0, -0.0, tiny, -tiny, np.finfo(dtype).tiny / 2, np.finfo(dtype).tiny, 5e-4, np.nextafter(t001, T(0)),
                     t001, np.nextafter(t001, T(1)), 0.5, 1.0, 3.25, 1e30, np.finfo(dtype).max, np.inf, -np.inf, np.nan,
                     -1.0, -5e-4, -1e30], dtype=dtype)


HIT_INDICES = np.array([0, 1, 498, 499, 500, 2 ** 31 - 1], dtype=np.uint32)


def hit_special_lists(dtype):
    """Candidate lists with a = 1 and disc = 0, so that both roots are -hb exactly: every (root, index) alone (the first
    candidate meets the initial state), every ordered pair (ties at equal t in both orders), and 2^15 random triples."""
    roots = special_roots(dtype)
    R, I = np.meshgrid(roots, HIT_INDICES, indexing="ij")
    R, I = R.ravel(), I.ravel()
    m = R.size
    one = (np.arange(m)[None, :], np.full(m, 1))
    a, b = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    two = (np.stack([a.ravel(), b.ravel()]), np.full(m * m, 2))
    rnd = np.random.default_rng(11)
    three = (rnd.integers(0, m, (3, 1 << 15)), np.full(1 << 15, 3))
    n = sum(p[1].size for p in (one, two, three))
    sel = np.zeros((8, n), np.int64)
    cnt = np.zeros(n, np.uint32)
    o = 0
    for pick, c in (one, two, three):
        sel[:pick.shape[0], o:o + c.size] = pick
        cnt[o:o + c.size] = c
        o += c.size
    hb = (-R[sel]).astype(dtype)
    return hb, np.zeros_like(hb), I[sel].astype(np.uint32), cnt, np.ones(n, dtype)


def hit_random_lists(dtype, n, seed):
    """Random candidate lists: 0..8 candidates, a in [0.5, 2), disc >= 0 (exact zeros included), a fifth of the
    candidates repeating the previous one's (hb, disc) under another index (ties)."""
    rnd = np.random.default_rng(seed)
    hb = rnd.uniform(-6.0, 2.0, (8, n)).astype(dtype)
    disc = rnd.uniform(0.0, 20.0, (8, n)).astype(dtype)
    disc[rnd.random((8, n)) < 0.05] = 0.0
    idx = rnd.integers(0, 2 ** 31, (8, n), dtype=np.int64).astype(np.uint32)
    small = rnd.random((8, n)) < 0.5
    idx[small] = rnd.integers(0, 8, int(small.sum())).astype(np.uint32)
    for c in range(1, 8):
        rep = rnd.random(n) < 0.2
        hb[c, rep], disc[c, rep] = hb[c - 1, rep], disc[c - 1, rep]
    cnt = rnd.integers(0, 9, n).astype(np.uint32)
    a = rnd.uniform(0.5, 2.0, n).astype(dtype)
    return hb, disc, idx, cnt, a


# ---------------------------------------------------------------- sincos2pi / unit_vec
def all_uniforms_f32():
    """Every uniform the fp32 RNG can produce: k * 2^-24."""
    return (np.arange(1 << 24, dtype=np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def uniforms_f64(n, seed):
    """n random 53-bit uniforms, plus every quadrant and octant boundary, its two neighbours on the RNG's grid
    (multiples of 2^-53) and as doubles, 0, and the ends."""
    rnd = np.random.default_rng(seed)
    u = (rnd.integers(0, 1 << 53, n, dtype=np.int64)).astype(np.float64) * 2.0 ** -53
    b = np.arange(0, 8, dtype=np.float64) / 8.0
    edge = np.concatenate([b, b + 2.0 ** -53, b[1:] - 2.0 ** -53, np.nextafter(b[1:], 1.0), np.nextafter(b[1:], 0.0),
                           [1.0 - 2.0 ** -53]])
    return np.concatenate([edge, u])


# ---------------------------------------------------------------- q8
def q8_dense_f64(n, seed):
    """n doubles dense around each quantisation boundary (k / 255.999)^2, k = 0..256."""
    rnd = np.random.default_rng(seed)
    k = rnd.integers(0, 257, n).astype(np.float64)
    x = (k / 255.999) ** 2
    ulps = rnd.integers(-64, 65, n)
    return np.abs((x.view(np.int64) + ulps).view(np.float64))
