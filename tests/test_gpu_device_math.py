"""The kernel's hand-written replacements for IEEE operations, run on their own on the GPU (tests/device/
rt_devunit.hip) and compared bit for bit with plain references: dvs (a shared refined v_rcp), sqrt_nd /
sqrt_len (v_sqrt_f32 + neighbour correction, v_rsq_f64 + Goldschmidt), HitBest<float> / hit_key, sincos2pi's
branch-free quadrant, div_dim's double product, the v_bitop3 Philox rounds.  The parity images exercise them
with ordinary arguments only; these tests go to the edges of each written precondition, put one
out-of-contract lane into otherwise clean waves (the ballot then moves 63 lanes to the other path), and feed
quotients and roots next to a rounding boundary.  The bar is 0 ulp: bit patterns, signed zeros included.

They pin the source-level sequences and the accuracy of the hardware's rcp / rsq / sqrt; the megakernel's own
code generation stays with the parity images.  Inputs and references: device_math_cases.py (checked on the CPU
by test_device_math_refs.py).
"""
import numpy as np
import pytest

import device_math_cases as dm
import devunit_bind as du
import oracle_bind as ob
from device_math_cases import assert_bits

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DT = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
BINADE = 1 << 23


def binade_f32(e, negative=False):
    """Every fp32 bit pattern of the binade [2^e, 2^(e+1))."""
    bits = np.arange(BINADE, dtype=np.uint32) + np.uint32(((e + 127) << 23) | (0x80000000 if negative else 0))
    return bits.view(F32)


# ---------------------------------------------------------------- a. fp32 sqrt, exhaustive
def test_sqrt_len_f32_every_bit_pattern():
    mis, first = du.sqrt_sweep_f32(0, 1 << 32, 0)
    assert mis == 0, [hex(b) for b in first]


def test_sqrt_len_f32_every_bit_pattern_mixed_waves():
    """Lane 7 of every odd wave holds a tiny positive argument: the other 63 lanes take the library path."""
    mis, first = du.sqrt_sweep_f32(0, 1 << 32, 1)
    assert mis == 0, [hex(b) for b in first]


def test_sqrt_nd_f32_every_pattern_in_contract():
    """+-0, [2^-96, +inf], [-inf, -2^-96] and every NaN: all patterns but the tiny nonzero ones of either sign."""
    lo = int(np.float32(2.0 ** -96).view(np.uint32))
    for start in (lo, lo | 0x80000000):
        mis, first = du.sqrt_sweep_f32(start, (1 << 31) - lo, 2)
        assert mis == 0, [hex(b) for b in first]
    x = np.array([0.0, -0.0, 2.0 ** -96, -2.0 ** -96, np.inf, -np.inf, np.nan, -1.0], F32)
    assert dm.sqrt_nd_in_contract(x).all()
    assert_bits(du.sqrt_nd(x), dm.ref_sqrt(x), "sqrt_nd specials", [x])


def test_sqrt_len_f32_negative_subnormals():
    """Regression: sqrt_len's ballot once sent only tiny positive arguments to the library sqrt, and sqrt_nd made -0,
    not NaN, of a negative subnormal (v_sqrt_f32 takes it as -0): all 2^23 - 1 of them, found by the exhaustive sweep."""
    x = (np.arange(1, BINADE, dtype=np.uint32) | np.uint32(0x80000000)).view(F32)
    assert np.isnan(dm.ref_sqrt(x)).all()
    assert_bits(du.sqrt_len(x), dm.ref_sqrt(x), "sqrt_len of negative subnormals", [x])
    x = np.array([-1e-45, -1e-40, -(2.0 ** -127), -(2.0 ** -126), -(2.0 ** -97), -(2.0 ** -96), -1.0] * 64, F32)
    assert_bits(du.sqrt_len(x), dm.ref_sqrt(x), "sqrt_len of small negatives", [x])


@pytest.mark.parametrize("binades", [(-97, -96), (-95, -24), (-1, 0), (1, 127)], ids=str)
def test_sqrt_len_f32_binades_on_the_host(binades):
    """The independent check of the device-side comparison: whole binades copied back and compared with numpy."""
    x = np.concatenate([binade_f32(e) for e in binades])
    ref = dm.ref_sqrt(x)
    assert_bits(ref, dm.ref_sqrt_via_f64(x), "numpy sqrt vs f64 sqrt rounded", [x])
    assert_bits(du.sqrt_len(x), ref, f"sqrt_len binades {binades}", [x])


def test_sqrt_len_f32_subnormals_specials_negatives():
    sub = np.arange(BINADE, dtype=np.uint32).view(F32)                  # +0 and every subnormal
    spec = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F32)
    x = np.concatenate([sub, binade_f32(0, negative=True), spec])
    assert_bits(du.sqrt_len(x), dm.ref_sqrt(x), "sqrt_len subnormals / negatives / specials", [x])
    x = np.concatenate([binade_f32(-96), spec])                         # no tiny lane: the short path
    assert_bits(du.sqrt_len(x), dm.ref_sqrt(x), "sqrt_len 2^-96 binade + specials", [x])


# ---------------------------------------------------------------- b. fp32 division at the rounding boundary
@pytest.fixture(scope="module")
def div_cases_f32():
    return dm.div_boundary_f32_all()


@pytest.mark.parametrize("es,ea", dm.DIV_PLACEMENTS_F32, ids=str)
def test_dvs_f32_rounding_boundary(div_cases_f32, es, ea):
    X, S, M, R = div_cases_f32
    v, s = dm.place_f32(X, S, es, ea)
    ref = dm.ref_div(v, s)
    assert_bits(ref, dm.predicted_quotient_f32(M, R, es, ea), "numpy quotient vs the construction's side")
    assert_bits(du.dvs(v, s), ref, f"dvs<float> boundary s=2^{es} a=2^{ea}", [v, s])


def test_dvs_f32_s_at_two_to_the_20(div_cases_f32):
    X = div_cases_f32[0][:1 << 20]
    for e in (20, 0, -100):
        v, s = dm.place_f32(X, X, 0, (e, e + 1, e))
        s = np.full_like(s, 2.0 ** 20)
        assert_bits(du.dvs(v, s), dm.ref_div(v, s), f"dvs<float> s = 2^20, a = 2^{e}", [v, s])
        s = np.full_like(s, 2.0 ** -20)
        assert_bits(du.dvs(v, s), dm.ref_div(v, s), f"dvs<float> s = 2^-20, a = 2^{e}", [v, s])


# ---------------------------------------------------------------- c. fp64 division and sqrt at the rounding boundary
@pytest.fixture(scope="module")
def div_cases_f64():
    return dm.div_boundary_f64(1 << 16, 5)


@pytest.mark.parametrize("es,ea", dm.DIV_PLACEMENTS_F64, ids=str)
def test_dvs_f64_rounding_boundary(div_cases_f64, es, ea):
    X, S, M, R = div_cases_f64
    v, s = dm.place_f64(X, S, es, ea)
    ref = dm.ref_div(v, s)
    assert_bits(ref, dm.predicted_quotient_f64(M, R, es, ea), "numpy quotient vs the construction's side")
    assert_bits(du.dvs(v, s), ref, f"dvs<double> boundary s=2^{es} a=2^{ea}", [v, s])


def test_sqrt_len_f64_rounding_boundary():
    x, exact = dm.sqrt_boundary_f64(1 << 16, 6)
    ref = dm.ref_sqrt(x)
    assert_bits(ref, exact, "numpy sqrt vs the integer square root")
    for sc in (0, -100, 98, -50):                                  # even scalings: the root scales exactly
        xs = np.ldexp(x, sc)
        assert_bits(du.sqrt_len(xs), np.ldexp(ref, sc // 2), f"sqrt_len<double> boundary * 2^{sc}", [xs])


BINADE_GROUPS = ((-100, -50), (-50, 0), (0, 50), (50, 100))


@pytest.mark.parametrize("lo,hi", BINADE_GROUPS, ids=str)
def test_sqrt_len_f64_random(lo, hi):
    x = np.concatenate([dm.random_binades(F64, 1 << 22, lo, hi, 100 + lo), [2.0 ** -100, 2.0 ** 100, 1.0, 4.0]])
    assert dm.sqrt_len_in_contract(x).all()
    assert_bits(du.sqrt_len(x), dm.ref_sqrt(x), f"sqrt_len<double> random 2^[{lo},{hi})", [x])


@pytest.mark.parametrize("lo,hi", ((-100, -50), (-50, 0), (0, 21)), ids=str)
def test_dvs_f64_random(lo, hi):
    n = 1 << 22
    v = np.stack([dm.random_binades(F64, n, lo, hi, 200 + lo + j, signed=True) for j in range(3)])
    s = dm.random_binades(F64, n, -20, 20, 300 + lo)
    s[:4] = [2.0 ** -20, 2.0 ** 20, 1.0, 2.0 ** 20]
    v[:, :2] = 2.0 ** -100
    assert dm.dvs_in_contract(v, s).all()
    assert_bits(du.dvs(v, s), dm.ref_div(v, s), f"dvs<double> random a in 2^[{lo},{hi})", [v, s])


def test_dvs_f32_random():
    n = 1 << 22
    for lo, hi in ((-100, -50), (-50, 0), (0, 21)):
        v = np.stack([dm.random_binades(F32, n, lo, hi, 400 + lo + j, signed=True) for j in range(3)])
        s = dm.random_binades(F32, n, -20, 20, 500 + lo)
        s[:4] = [2.0 ** -20, 2.0 ** 20, 1.0, 2.0 ** 20]
        v[:, :2] = 2.0 ** -100
        assert dm.dvs_in_contract(v, s).all()
        ref = dm.ref_div(v, s)
        assert_bits(ref, dm.ref_div_via_f64(v, s), "numpy quotient vs f64 quotient rounded")
        assert_bits(du.dvs(v, s), ref, f"dvs<float> random a in 2^[{lo},{hi})", [v, s])


# ---------------------------------------------------------------- d. contract edges and mixed waves
def _dvs_base(dtype, n=1 << 16):
    v = np.stack([dm.random_binades(dtype, n, -30, 2, 600 + j, signed=True) for j in range(3)])
    s = dm.random_binades(dtype, n, -2, 4, 610)
    return v, s


@DT
@pytest.mark.parametrize("what", ["s=2^21", "s=2^-21", "s<0", "a=2^-101", "a=0", "a=-0"])
def test_dvs_mixed_waves(dtype, what):
    """Run A: every lane in contract.  Run B: lane 7 of every odd wave out of contract; the whole wave then takes the
    IEEE division.  Both equal the reference, and the untouched lanes agree between the runs."""
    T = np.dtype(dtype).type
    v, s = _dvs_base(dtype)
    assert dm.waves_all(dm.dvs_in_contract(du.pad(v, 1.0), du.pad(s, 1.0))).all()
    vb, sb = v.copy(), s.copy()
    if what.startswith("s"):
        sb = dm.break_lane7(s, {"s=2^21": T(2.0 ** 21), "s=2^-21": T(2.0 ** -21), "s<0": T(-1.5)}[what])
    else:
        vb[1] = dm.break_lane7(v[1], {"a=2^-101": T(2.0 ** -101), "a=0": T(0.0), "a=-0": T(-0.0)}[what])
    broke = dm.broken_lanes(s.size)
    ok = dm.waves_all(dm.dvs_in_contract(vb, sb))
    assert not ok[1::2].any() and ok[0::2].all()
    ga, gb = du.dvs(v, s), du.dvs(vb, sb)
    assert_bits(ga, dm.ref_div(v, s), f"dvs {what} run A", [v, s])
    assert_bits(gb, dm.ref_div(vb, sb), f"dvs {what} run B", [vb, sb])
    assert_bits(gb[:, ~broke], ga[:, ~broke], f"dvs {what}: untouched lanes, run B vs run A")


@DT
def test_sqrt_len_mixed_waves(dtype):
    T = np.dtype(dtype).type
    x = dm.random_binades(dtype, 1 << 16, -90, 90, 620)
    assert dm.waves_all(dm.sqrt_len_in_contract(du.pad(x, 1.0))).all()
    ga = du.sqrt_len(x)
    assert_bits(ga, dm.ref_sqrt(x), "sqrt_len run A", [x])
    broke = dm.broken_lanes(x.size)
    outs = [2.0 ** -100, 2.0 ** -149, 2.0 ** -127, -(2.0 ** -100), -(2.0 ** -149)] if dtype is F32 else [2.0 ** -101, 2.0 ** 101, 0.0, -1.0, np.inf, np.nan, 5e-324]
    for bad in outs:
        xb = dm.break_lane7(x, T(bad))
        ok = dm.waves_all(dm.sqrt_len_in_contract(xb))
        assert not ok[1::2].any() and ok[0::2].all()
        gb = du.sqrt_len(xb)
        assert_bits(gb, dm.ref_sqrt(xb), f"sqrt_len run B ({bad})", [xb])
        assert_bits(gb[~broke], ga[~broke], f"sqrt_len ({bad}): untouched lanes, run B vs run A")


@DT
def test_dvs_large_quotients(dtype):
    """next_ray's scalar mode divides p - c by the radius: a small sphere far from the origin has |a_i| / s up to
    2^40, inside dvs's written contract (which bounds s and the smallest component only)."""
    n = 1 << 20
    v = np.stack([dm.random_binades(dtype, n, -20, 21, 630 + j, signed=True) for j in range(3)])
    s = dm.random_binades(dtype, n, -20, 20, 640)
    s[:2], v[:, :2] = 2.0 ** -20, 2.0 ** 20
    assert dm.dvs_in_contract(v, s).all()
    assert_bits(du.dvs(v, s), dm.ref_div(v, s), "dvs, |a| / s up to 2^40", [v, s])


@DT
def test_dvs_largest_reachable_quotients(dtype):
    """The bound of DESIGN.md section 2 on the scalar mode's |vec_i| / radius: components up to 2^89 over s down to
    2^-20 (quotients up to 2^110), in fp64 up to 2^600 over 2^-20; far from ordinary, but inside the contract."""
    n = 1 << 18
    top = 90 if dtype is F32 else 601
    v = np.stack([dm.random_binades(dtype, n, 30, top, 650 + j, signed=True) for j in range(3)])
    s = dm.random_binades(dtype, n, -20, 1, 660)
    s[:2] = 2.0 ** -20
    assert dm.dvs_in_contract(v, s).all()
    ref = dm.ref_div(v, s)
    assert np.isfinite(ref).all()
    assert_bits(du.dvs(v, s), ref, "dvs, the largest reachable quotients", [v, s])


# Outside dvs's reachable inputs: a quotient that overflows.  The fast path gives NaN where the
# IEEE division gives +-inf (m = inf, fma(-s, inf, x) = -inf, fma(-inf, r1, inf) = NaN).  fp32 needs |a_i| > 2^108 with
# s <= 2^20; every caller forms len2 or a discriminant from the same components first, which overflows (|a_i|^2 > 2^216)
# and is NaN / inf long before.  Recorded, not asserted.
# Measured on an MI355X: (2^120, -2^120, 1) / 2^-10 gives (NaN, NaN, 1024) in fp32, (2^1010, -2^1010, 1) / 2^-15 gives
# (NaN, NaN, 32768) in fp64; the IEEE quotients are (+inf, -inf, .).
OUTSIDE_THE_CONTRACT = {"dvs<float> overflowing quotient": (np.float32(2.0 ** 120), np.float32(2.0 ** -10)),
                        "dvs<double> overflowing quotient": (2.0 ** 1010, 2.0 ** -15)}


# ---------------------------------------------------------------- e. unit
@DT
def test_unit_random_vectors(dtype):
    v = dm.random_vectors(dtype, 1 << 22, -30, 30, 700)
    ref = dm.ref_unit(v)
    assert_bits(ob.oracle_unit(v), ref, "oracle unit vs numpy")
    assert_bits(du.unit(v), ref, "unit, exponents in [-30, 30]", [v])


@DT
def test_unit_needles(dtype):
    v = dm.needle_vectors(dtype, 1 << 20, 710)
    assert_bits(du.unit(v), dm.ref_unit(v), "unit, one dominant axis", [v])


@DT
def test_unit_fallbacks(dtype):
    """Zero components and a squared length that overflows or underflows: the ballot's IEEE path."""
    big, small = (64, -70) if dtype is F32 else (512, -530)
    n = 1 << 14
    parts = [dm.random_vectors(dtype, n, -4, 4, 720), dm.random_vectors(dtype, n, -4, 4, 721),
             dm.random_vectors(dtype, n, big, big + 6, 722), dm.random_vectors(dtype, n, small - 6, small, 723),
             dm.random_vectors(dtype, n, -4, 4, 724)]
    parts[0][1] = 0.0
    parts[1][0], parts[1][2] = -0.0, 0.0
    parts[4][:, ::3] = 0.0                                             # the zero vector: NaN
    v = np.concatenate(parts, axis=1)
    v = v[:, np.random.default_rng(725).permutation(v.shape[1])]      # mixed waves
    assert_bits(du.unit(v), dm.ref_unit(v), "unit, zero components / len2 out of range", [v])


# ---------------------------------------------------------------- f. sincos2pi, unit_vec, refract
def test_sincos2pi_f32_every_uniform():
    u = dm.all_uniforms_f32()
    s, c = du.sincos2pi(u)
    rs, rc = ob.oracle_sincos2pi(u)
    assert_bits(s, rs, "sin(2 pi u), every fp32 uniform", [u])
    assert_bits(c, rc, "cos(2 pi u), every fp32 uniform", [u])


def test_sincos2pi_f64():
    u = dm.uniforms_f64(1 << 22, 800)
    s, c = du.sincos2pi(u)
    rs, rc = ob.oracle_sincos2pi(u)
    assert_bits(s, rs, "sin(2 pi u) f64", [u])
    assert_bits(c, rc, "cos(2 pi u) f64", [u])


@pytest.mark.parametrize("full_arg", [1, 2])
def test_unit_vec_f32_full_range(full_arg):
    """The full range of one uniform against 64 values of the other (interleaved, so the 64 alternate along the range)."""
    u = dm.all_uniforms_f32()
    rnd = np.random.default_rng(810)
    other = np.concatenate([[0.0, 0.25, 0.5, 0.75, 0.125, 1 - 2.0 ** -24, 2.0 ** -24, 0.5 - 2.0 ** -24],
                            rnd.integers(0, 1 << 24, 56) * 2.0 ** -24]).astype(F32)
    o = other[np.arange(u.size) % 64]
    u1, u2 = (u, o) if full_arg == 1 else (o, u)
    assert_bits(du.unit_vec(u1, u2), ob.oracle_unit_vec(u1, u2), f"unit_vec<float>, full range in u{full_arg}", [u1, u2])


def test_unit_vec_f64():
    u1, u2 = dm.uniforms_f64(1 << 22, 820), dm.uniforms_f64(1 << 22, 821)[::-1].copy()
    assert_bits(du.unit_vec(u1, u2), ob.oracle_unit_vec(u1, u2), "unit_vec<double>", [u1, u2])


@DT
def test_refract(dtype):
    n = 1 << 20
    v = dm.ref_unit(dm.random_vectors(dtype, n, -2, 2, 830))
    nrm = dm.ref_unit(dm.random_vectors(dtype, n, -2, 2, 831))
    ratio = np.random.default_rng(832).choice(np.array([1.5, 1 / 1.5, 1.0, 2.4, 1 / 2.4, 1.33, 1 / 1.33]), n).astype(dtype)
    v[:, :64], nrm[:, :64] = np.array([[0.0], [-1.0], [0.0]]), np.array([[0.0], [1.0], [0.0]])   # head-on: |1 - len2| = 1
    assert_bits(du.refract(v, nrm, ratio), ob.oracle_refract(v, nrm, ratio), "refract", [v, nrm, ratio])


# ---------------------------------------------------------------- g. hit_update
@DT
@pytest.mark.parametrize("mode", ["packed", "root2", "scalar"])
def test_hit_update_special_roots(dtype, mode):
    hb, disc, idx, cnt, a = dm.hit_special_lists(dtype)
    t, i = du.hit(hb, disc, idx, cnt, a, mode)
    rt_, ri = dm.ref_hit(hb, disc, idx, cnt, a, mode)
    assert_bits(i, ri, f"hit_update<{mode}> index, special roots", [hb, idx, cnt])
    assert_bits(t, rt_, f"hit_update<{mode}> t, special roots", [hb, idx, cnt])


@DT
@pytest.mark.parametrize("mode", ["packed", "root2", "scalar"])
def test_hit_update_random_lists(dtype, mode):
    hb, disc, idx, cnt, a = dm.hit_random_lists(dtype, 1 << 20, 900)
    t, i = du.hit(hb, disc, idx, cnt, a, mode)
    rt_, ri = dm.ref_hit(hb, disc, idx, cnt, a, mode)
    assert (ri >= 0).mean() > 0.5                                      # most lists do hit
    assert_bits(i, ri, f"hit_update<{mode}> index, random lists", [hb, disc, idx, cnt, a])
    assert_bits(t, rt_, f"hit_update<{mode}> t, random lists", [hb, disc, idx, cnt, a])


# ---------------------------------------------------------------- h. div_dim
@pytest.mark.parametrize("W", [1, 2, 3, 7, 400, 1920, 3840, 65535])
def test_div_dim_f32(W):
    u = dm.all_uniforms_f32()
    r = dm.host_rW(W)
    assert r != 0.0
    for col in sorted({0, W // 2, W - 1}):
        x = (F32(col) + u).astype(F32)                                  # (T)col + u01a, rt_camera.hpp
        ref = dm.ref_div_dim(x, W)
        assert_bits(du.div_dim(x, W, r), ref, f"div_dim<float> W={W} col={col}", [x])
    sub = u[np.linspace(0, u.size - 1, max(1, (1 << 22) // W)).astype(np.int64)]
    x = (np.arange(W, dtype=F32)[:, None] + sub[None, :]).ravel()      # every column
    assert_bits(du.div_dim(x, W, r), dm.ref_div_dim(x, W), f"div_dim<float> W={W}, every column", [x])
    assert_bits(du.div_dim(x, W, 0.0), dm.ref_div_dim(x, W), f"div_dim<float> W={W}, r = 0 (plain division)", [x])


def test_div_dim_f64_and_large():
    rnd = np.random.default_rng(910)
    for W in (1, 3, 400, 3840, 65535, (1 << 20) + 1):
        x = (rnd.integers(0, W, 1 << 18) + rnd.random(1 << 18)).astype(F64)
        assert_bits(du.div_dim(x, W, dm.host_rW(W)), dm.ref_div_dim(x, W), f"div_dim<double> W={W}", [x])
    W = (1 << 20) + 1                                                   # the host sets r = 0 from 2^20 on
    x = (rnd.integers(0, W, 1 << 20).astype(F32) + dm.all_uniforms_f32()[::16]).astype(F32)
    assert dm.host_rW(W) == 0.0
    assert_bits(du.div_dim(x, W, 0.0), dm.ref_div_dim(x, W), "div_dim<float> W = 2^20 + 1", [x])


# ---------------------------------------------------------------- i. q8
Q8_TOP = int(np.float32(4.0).view(np.uint32)) + 1       # patterns 0 .. bits(4.0f)
Q8_SLAB = 1 << 24


@pytest.mark.parametrize("first", range(0, -(-Q8_TOP // Q8_SLAB), 8))
def test_q8_f32_every_pattern_up_to_4(first):
    for slab in range(first, min(first + 8, -(-Q8_TOP // Q8_SLAB))):
        v = np.arange(slab * Q8_SLAB, min((slab + 1) * Q8_SLAB, Q8_TOP), dtype=np.uint32).view(F32)
        assert_bits(du.q8(v), dm.ref_q8(v), f"q8<float> slab {slab}", [v])


def test_q8_negatives_specials_f64():
    v = np.concatenate([-dm.random_binades(F32, 1 << 16, -140, 3, 920), [np.nan, np.inf, -np.inf, -0.0, 0.0, 4.0, 1e30]]).astype(F32)
    assert_bits(du.q8(v), dm.ref_q8(v), "q8<float> negatives / NaN / inf", [v])
    v = np.concatenate([dm.q8_dense_f64(1 << 22, 921), [np.nan, np.inf, -np.inf, -0.0, 0.0, 4.0, -1.0]])
    ref = dm.ref_q8(v)
    assert_bits(ob.oracle_q8(v), ref, "oracle q8 vs numpy")
    assert_bits(du.q8(v), ref, "q8<double> around every boundary", [v])


# ---------------------------------------------------------------- j. RNG
def test_philox_published_vectors_on_the_device():
    """Random123's kat_vectors for philox4x32 and philox2x32, R = 10, through the device's v_bitop3 rounds."""
    ctr = np.array([[0] * 4, [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32).T
    key = np.array([[0, 0], [0xFFFFFFFF] * 2, [0xA4093822, 0x299F31D0]], np.uint32).T
    want = np.array([[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
                     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]], np.uint32).T
    assert np.array_equal(du.philox4x32_10(ctr, key), want)
    ctr2 = np.array([[0, 0], [0xFFFFFFFF] * 2, [0x243F6A88, 0x85A308D3]], np.uint32).T
    key2 = np.array([0, 0xFFFFFFFF, 0x13198A2E], np.uint32)
    want2 = np.array([[0xFF1DAE59, 0x6CD10DF2], [0x2C3F628B, 0xAB4FD7AD], [0xDD7CE038, 0xF62A4C12]], np.uint32).T
    assert np.array_equal(du.philox2x32_10(ctr2, key2), want2)


SEEDS = (0, 0x5EED0001, 0x100000001, 0xDEADBEEF5EED0001, 0xFFFFFFFFFFFFFFFF)


@DT
def test_rng_counter_ends_and_random(dtype):
    from rt_mi355x.abi import RT_MAX_BOUNCES_F32
    ends = np.array(np.meshgrid([0, (1 << 20) - 1], [0, (1 << 32) - 1], [0, 255, RT_MAX_BOUNCES_F32 - 1], [0, 1, 2],
                                indexing="ij"), dtype=np.uint64).reshape(4, -1)
    rnd = np.random.default_rng(930)
    n = 1 << 20
    rand = np.stack([rnd.integers(0, 1 << 20, n), rnd.integers(0, 1 << 32, n), rnd.integers(0, RT_MAX_BOUNCES_F32, n),
                     rnd.integers(0, 3, n)]).astype(np.uint64)
    rand[2, rand[3] == 0] = 0                                            # the camera stream draws k = 0 only
    rand[2, rand[3] == 1] &= 255                                         # disk tries: 1 + k < 257
    ends = ends[:, ~((ends[3] == 0) & (ends[2] != 0)) & ~((ends[3] == 1) & (ends[2] > 255))]
    sid, pix, k, stream = np.concatenate([ends, rand], axis=1).astype(np.uint32)
    for seed in SEEDS:
        r, ua, ub = du.rng(dtype, sid, pix, k, stream, seed)
        wr, wa, wb = ob.oracle_draw(dtype, sid, pix, k, stream, seed)
        assert np.array_equal(r, wr), f"rng block, seed {seed:#x}"
        assert_bits(ua, wa, f"u01a, seed {seed:#x}")
        assert_bits(ub, wb, f"u01b, seed {seed:#x}")
