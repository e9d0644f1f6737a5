"""CPU checks of the inputs and references that tests/test_gpu_device_math.py feeds to the GPU
(device_math_cases.py): the generators produce the counts and the hardness they claim, every "in-contract"
family satisfies the written precondition on every lane of every wave after padding, the numpy references
agree with the oracle's probes wherever both exist, and the oracle's new probes agree with the independent
restatement.  No GPU is involved: a failure here is a fault of the test material, not of the kernel.
"""
from fractions import Fraction

import numpy as np
import pytest

import device_math_cases as dm
import devunit_bind as du
import independent_v2 as iv
import oracle_bind as ob
from device_math_cases import assert_bits

F32, F64 = np.float32, np.float64
DT = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])


# ---------------------------------------------------------------- fp32 division next to a rounding boundary
@pytest.fixture(scope="module")
def div_cases_f32():
    return dm.div_boundary_f32_all()


def test_div_boundary_f32_counts_and_hardness(div_cases_f32):
    X, S, M, R = div_cases_f32
    for r in dm.DIV_R:
        sel = R == r
        assert sel.sum() >= 10 ** 6, (r, int(sel.sum()))
        x, s, m = (a[sel].astype(object) for a in (X, S, M))          # Python integers: exact
        assert ((s * m - r) == (x << 25)).all()                        # X = (S*M - r) / 2^25 exactly
        assert (s % 2 == 1).all() and (m % 2 == 1).all()               # M odd: M / 2^25 is a float midpoint
        assert (m >= 1 << 24).all() and (m < 1 << 25).all() and (x >= 1 << 23).all() and (x < 1 << 24).all()
    # The relative distance of X / S from the midpoint M / 2^25 is |r| / (S * M), and X >= 2^23 means
    # S * M >= 2^48 + r: at most 2^-48 (inside 2^-47) for r = +-1 and 3 * 2^-48 = 1.5 * 2^-47 for r = +-3 -- the
    # construction cannot do better for |r| = 3 (about 287 000 of its 1.29 million cases lie inside 2^-47).
    SM = S.astype(object) * M.astype(object)
    assert (SM >= (1 << 48) + R.astype(object)).all()
    dist = np.abs(R).astype(F64) / (S.astype(F64) * M.astype(F64))
    one = np.abs(R) == 1
    assert dist[one].max() <= 2.0 ** -47 and dist[one].max() <= 2.0 ** -48 * (1 + 1e-12), dist[one].max()
    assert dist[~one].max() <= 3 * 2.0 ** -48 * (1 + 1e-12), dist[~one].max()


@pytest.mark.parametrize("es,ea", dm.DIV_PLACEMENTS_F32, ids=str)
def test_div_boundary_f32_reference_rounds_to_the_predicted_side(div_cases_f32, es, ea):
    X, S, M, R = div_cases_f32
    v, s = dm.place_f32(X, S, es, ea)
    assert dm.waves_all(dm.dvs_in_contract(du.pad(v, 1.0), du.pad(s, 1.0))).all()
    assert (np.abs(v) <= s).all()                                      # unit()'s situation: |a_i| <= len
    ref = dm.ref_div(v, s)
    assert_bits(ref, dm.predicted_quotient_f32(M, R, es, ea), "numpy quotient vs the construction's side")
    assert_bits(ref, dm.ref_div_via_f64(v, s), "numpy quotient vs f64 quotient rounded")


def test_smallest_component_sits_at_the_contract_edge(div_cases_f32):
    X, S = div_cases_f32[0][:4096], div_cases_f32[1][:4096]
    for es, ea in dm.DIV_PLACEMENTS_F32:
        v, s = dm.place_f32(X, S, es, ea)
        lo = np.abs(v).min(axis=0)
        assert (lo >= F32(2.0 ** min(ea))).all() and (lo < F32(2.0 ** (min(ea) + 1))).all()
        assert (s >= F32(2.0 ** es)).all() and (s < F32(2.0 ** (es + 1))).all()
    assert min(min(ea) for _, ea in dm.DIV_PLACEMENTS_F32) == -100
    assert {es for es, _ in dm.DIV_PLACEMENTS_F32} == {-20, 0, 19}


# ---------------------------------------------------------------- fp64 division / sqrt next to a rounding boundary
@pytest.fixture(scope="module")
def div_cases_f64():
    return dm.div_boundary_f64(1 << 16, 5)


def test_div_boundary_f64(div_cases_f64):
    X, S, M, R = div_cases_f64
    assert X.size == 1 << 16 and set(np.unique(R)) == set(dm.DIV_R)
    for x, s, m, r in list(zip(X.tolist(), S.tolist(), M.tolist(), R.tolist()))[::64]:
        assert s * m - r == x << 54 and m & 1 and s & 1
        assert abs(Fraction(x, s) - Fraction(m, 1 << 54)) / Fraction(m, 1 << 54) <= Fraction(1, 1 << 104)
    for es, ea in dm.DIV_PLACEMENTS_F64:
        v, s = dm.place_f64(X, S, es, ea)
        assert dm.waves_all(dm.dvs_in_contract(du.pad(v, 1.0), du.pad(s, 1.0))).all()
        assert_bits(dm.ref_div(v, s), dm.predicted_quotient_f64(M, R, es, ea), "numpy quotient vs the construction's side")


def test_sqrt_boundary_f64():
    x, exact = dm.sqrt_boundary_f64(1 << 12, 6)
    assert x.size >= (1 << 13) - 8 and (x >= 1.0).all() and (x < 4.0).all()
    assert_bits(dm.ref_sqrt(x), exact, "numpy sqrt vs the integer square root")
    # hardness: the exact root lies within 2^-53 relative of the midpoint of two doubles
    for xv in x[:256].tolist():
        X = Fraction(xv)
        lo = Fraction(float(np.sqrt(xv)))
        mids = [lo - Fraction(float(np.spacing(float(lo)))) / 2, lo + Fraction(float(np.spacing(float(lo)))) / 2]
        gap = min(abs(m * m - X) / (2 * m) for m in mids)              # |sqrt(X) - m| ~ |X - m^2| / 2m
        assert gap / lo <= Fraction(1, 1 << 53), float(gap / lo)
    for sc in (0, -100, 98, -50):
        assert dm.sqrt_len_in_contract(np.ldexp(x, sc)).all()
        assert_bits(dm.ref_sqrt(np.ldexp(x, sc)), np.ldexp(exact, sc // 2), "scaled roots")


def test_exact_sqrt_f64_on_known_values():
    assert dm.exact_sqrt_f64(4, 0) == 2.0 and dm.exact_sqrt_f64(1, -2) == 0.5 and dm.exact_sqrt_f64(9, 3) == np.sqrt(72.0)
    rnd = np.random.default_rng(1)
    for m in rnd.integers(1 << 52, 1 << 53, 500).tolist():
        for e in (-52, -51, 0, 7):
            assert dm.exact_sqrt_f64(m, e) == np.sqrt(np.ldexp(float(m), e))


# ---------------------------------------------------------------- contracts, padding, mixed waves
@DT
def test_padding_is_inside_every_contract(dtype):
    T = np.dtype(dtype).type
    v, s, x = np.full((3, 1), T(0.5)), np.full(1, T(2.0)), np.full(1, T(3.0))
    vp, sp, xp = du.pad(v, 1.0), du.pad(s, 1.0), du.pad(x, 1.0)
    assert vp.shape == (3, 256) and sp.shape == (256,) and vp.dtype == dtype
    assert dm.dvs_in_contract(vp, sp).all() and dm.sqrt_len_in_contract(xp).all()
    assert dm.sqrt_len_in_contract(dm.ref_len2(vp)).all()              # unit()'s padding
    assert du.pad(np.zeros(256, dtype), 1.0).size == 256 and du.pad(np.zeros(257, dtype), 1.0).size == 512


@DT
def test_contract_edges(dtype):
    T = np.dtype(dtype).type
    one = np.ones((3, 1), dtype)
    for sv, ok in ((2.0 ** -20, True), (2.0 ** 20, True), (2.0 ** 21, False), (2.0 ** -21, False), (-1.5, False),
                   (np.nextafter(T(2.0 ** 20), T(np.inf)), False), (np.nextafter(T(2.0 ** -20), T(0)), False)):
        assert dm.dvs_in_contract(one, np.array([sv], dtype))[0] == ok, sv
    for av, ok in ((2.0 ** -100, True), (-2.0 ** -100, True), (2.0 ** -101, False), (0.0, False), (-0.0, False)):
        v = one.copy()
        v[2] = av
        assert dm.dvs_in_contract(v, np.ones(1, dtype))[0] == ok, av
    if dtype is F32:
        cases = ((2.0 ** -96, True), (2.0 ** -100, False), (2.0 ** -149, False), (0.0, True), (-0.0, True), (-1.0, True),
                 (np.inf, True), (np.nan, True), (-2.0 ** -96, True), (-2.0 ** -97, False), (-1e-45, False))
    else:
        cases = ((2.0 ** -100, True), (2.0 ** 100, True), (2.0 ** -101, False), (2.0 ** 101, False), (0.0, False), (np.nan, False))
    for xv, ok in cases:
        assert dm.sqrt_len_in_contract(np.array([xv], dtype))[0] == ok, xv


def test_broken_lane_is_lane_7_of_every_odd_wave():
    x = np.ones(64 * 6, F32)
    b = dm.break_lane7(x, F32(9.0))
    assert np.flatnonzero(b == 9.0).tolist() == [64 + 7, 3 * 64 + 7, 5 * 64 + 7]
    assert np.array_equal(dm.broken_lanes(x.size), b == 9.0) and (x == 1.0).all()
    ok = dm.waves_all(b == 1.0)
    assert ok.tolist() == [True, False] * 3


@DT
def test_random_families_are_in_contract(dtype):
    x = dm.random_binades(dtype, 1 << 16, -90, 90, 620)
    assert dm.sqrt_len_in_contract(x).all() and (x > 0).all()
    assert np.log2(x.astype(F64)).min() >= -90 and np.log2(x.astype(F64)).max() < 90
    v = np.stack([dm.random_binades(dtype, 1 << 16, -100, -50, j, signed=True) for j in range(3)])
    s = dm.random_binades(dtype, 1 << 16, -20, 20, 3)
    assert dm.dvs_in_contract(v, s).all() and (v < 0).any() and (v > 0).any()


# ---------------------------------------------------------------- numpy references against the oracle
@DT
def test_numpy_unit_and_q8_equal_the_oracle(dtype):
    v = np.concatenate([dm.random_vectors(dtype, 1 << 16, -30, 30, 700), dm.needle_vectors(dtype, 1 << 14, 710)], axis=1)
    assert_bits(ob.oracle_unit(v), dm.ref_unit(v), "oracle unit vs numpy")
    x = np.concatenate([dm.q8_dense_f64(1 << 16, 921).astype(dtype), np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 4.0, -1.0], dtype),
                        dm.random_binades(dtype, 1 << 14, -20, 3, 5)])
    assert_bits(ob.oracle_q8(x), dm.ref_q8(x), "oracle q8 vs numpy")


def test_q8_dense_sits_on_the_boundaries():
    x = dm.q8_dense_f64(1 << 16, 921)
    q = dm.ref_q8(x[np.isfinite(x)])
    assert len(np.unique(q)) == 256                                    # every output value occurs
    k = np.rint(np.sqrt(x[np.isfinite(x)]) * 255.999)
    assert np.abs(np.sqrt(x[np.isfinite(x)]) * 255.999 - k).max() < 1e-9


@DT
def test_numpy_hit_rule_equals_the_key_rule_of_test_device_bits(dtype):
    """ref_hit, folded over one candidate against a given best, is the rule test_device_bits.py states."""
    roots = dm.special_roots(dtype)
    t001 = np.dtype(dtype).type(0.001)
    for bt, bi in ((1.0, 7), (0.001, 0), (3.25, 499)):
        for i in dm.HIT_INDICES:
            hb = np.zeros((8, roots.size), dtype)
            hb[0], hb[1] = -np.dtype(dtype).type(bt), -roots
            idx = np.zeros((8, roots.size), np.uint32)
            idx[0], idx[1] = bi, i
            cnt, a = np.full(roots.size, 2, np.uint32), np.ones(roots.size, dtype)
            t, j = dm.ref_hit(hb, np.zeros_like(hb), idx, cnt, a, "packed")
            with np.errstate(invalid="ignore"):
                valid = (roots >= t001) & (roots < np.inf)
                take = valid & ((roots < bt) | ((roots == bt) & (int(i) > bi)))
            assert np.array_equal(j, np.where(take, np.int32(i), np.int32(bi)))
            assert_bits(t, np.where(take, roots, np.dtype(dtype).type(bt)), "t")
            t, j = dm.ref_hit(hb, np.zeros_like(hb), idx, cnt, a, "scalar")
            take = valid & ((roots < bt) | ((roots == bt) & (int(i) < bi)))
            assert np.array_equal(j, np.where(take, np.int32(i), np.int32(bi)))


@DT
def test_hit_lists(dtype):
    hb, disc, idx, cnt, a = dm.hit_special_lists(dtype)
    m = dm.special_roots(dtype).size * dm.HIT_INDICES.size
    assert hb.shape == (8, m + m * m + (1 << 15)) and (disc == 0).all() and (a == 1).all()
    assert (cnt[:m] == 1).all() and (cnt[m:m + m * m] == 2).all() and (cnt[m + m * m:] == 3).all()
    two = slice(m, m + m * m)
    tie = (hb[0, two] == hb[1, two]) & (idx[0, two] != idx[1, two]) & (-hb[0, two] >= 0.001) & np.isfinite(hb[0, two])
    assert tie.sum() >= 2 * 30                                         # ties at equal t, in both orders
    assert {0, 1, 498, 499, 500, 2 ** 31 - 1} == set(dm.HIT_INDICES.tolist())
    t, i = dm.ref_hit(hb, disc, idx, cnt, a, "packed")
    assert (i[:m] == -1).any() and (i[:m] >= 0).any() and np.isinf(t[i == -1]).all()
    hb, disc, idx, cnt, a = dm.hit_random_lists(dtype, 1 << 14, 900)
    assert cnt.min() == 0 and cnt.max() == 8 and (disc >= 0).all() and (disc == 0).any()
    for mode in ("packed", "root2", "scalar"):
        t, i = dm.ref_hit(hb, disc, idx, cnt, a, mode)
        assert 0.5 < (i >= 0).mean() < 1.0
    assert ((hb[1:] == hb[:-1]) & (disc[1:] == disc[:-1])).mean() > 0.1   # repeated candidates: ties


# ---------------------------------------------------------------- the oracle's new probes
def test_oracle_sincos2pi_f32_equals_the_independent_restatement():
    import random
    rng = random.Random(3)
    us = [0.0, 0.125, 0.25, 0.5, 0.75, 1 - 2 ** -24] + [rng.randrange(1 << 24) / (1 << 24) for _ in range(2000)]
    u = np.array(us, F32)
    s, c = ob.oracle_sincos2pi(u)
    for j, uv in enumerate(u):
        ws, wc = iv.sincos2pi(iv.F32(uv))
        assert (F32(ws).view(np.uint32), F32(wc).view(np.uint32)) == (s[j].view(np.uint32), c[j].view(np.uint32)), uv


def test_oracle_sincos2pi_f64_batched_equals_the_scalar_probe():
    import ctypes
    lib = ob.load_oracle()
    u = dm.uniforms_f64(2000, 800)
    s, c = ob.oracle_sincos2pi(u)
    a, b = ctypes.c_double(), ctypes.c_double()
    for j, uv in enumerate(u.tolist()):
        lib.oracle_sincos2pi_f64(uv, ctypes.byref(a), ctypes.byref(b))
        assert (a.value, b.value) == (s[j], c[j]) and iv.sincos2pi(uv) == (s[j], c[j]), uv


def test_uniform_sets():
    u = dm.all_uniforms_f32()
    assert u.size == 1 << 24 and u[0] == 0 and u[-1] == F32(1 - 2.0 ** -24) and (np.diff(u) == F32(2.0 ** -24)).all()
    u = dm.uniforms_f64(1000, 1)
    assert (u >= 0).all() and (u < 1).all()
    for b in np.arange(8) / 8.0:
        assert b in u and b + 2.0 ** -53 in u and (b == 0 or (b - 2.0 ** -53 in u and np.nextafter(b, 0.0) in u))


@DT
def test_oracle_draw_probe(dtype):
    """draw + u01 against the oracle's own Philox blocks and the uniform mapping written out."""
    import ctypes
    lib = ob.load_oracle()
    sid = np.array([0, 5, (1 << 20) - 1, 17], np.uint32)
    pix = np.array([0, 9, (1 << 32) - 1, 123456], np.uint32)
    k = np.array([0, 3, 255, 3838], np.uint32)
    stream = np.array([0, 1, 1, 2], np.uint32)
    for seed in (0x5EED0001, 0xDEADBEEF5EED0001):
        r, ua, ub = ob.oracle_draw(dtype, sid, pix, k, stream, seed)
        for j in range(4):
            if dtype is F64:
                out = (ctypes.c_uint32 * 4)()
                lib.oracle_philox4x32_10((ctypes.c_uint32 * 4)(int(sid[j]), int(pix[j]), int(k[j]), int(stream[j])),
                                         (ctypes.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32), out)
                assert list(out) == r[:, j].tolist()
                assert ua[j] == float(((out[0] << 32) | out[1]) >> 11) * 2.0 ** -53
                assert ub[j] == float(((out[2] << 32) | out[3]) >> 11) * 2.0 ** -53
            else:
                code = [0, 1 + int(k[j]), 257 + int(k[j])][int(stream[j])]
                out = (ctypes.c_uint32 * 2)()
                key = (seed & 0xFFFFFFFF) ^ lib.oracle_fmix32(seed >> 32)
                lib.oracle_philox2x32_10((ctypes.c_uint32 * 2)(int(pix[j]), int(sid[j]) | (code << 20)), key, out)
                assert list(out) + [0, 0] == r[:, j].tolist()
                assert ua[j] == F32(out[0] >> 8) * F32(2.0 ** -24) and ub[j] == F32(out[1] >> 8) * F32(2.0 ** -24)
        assert (ua >= 0).all() and (ua < 1).all() and (ub >= 0).all() and (ub < 1).all()


@DT
def test_oracle_unit_vec_and_refract_probes(dtype):
    """The batched probes are the oracle's own functions: unit_vec from its sincos2pi probe, refract's formula in numpy
    (no FMA in it: geometry.rs:183-188)."""
    T = np.dtype(dtype).type
    rnd = np.random.default_rng(4)
    scale = 2.0 ** -24 if dtype is F32 else 2.0 ** -53
    u1 = (rnd.integers(0, int(1 / scale), 4096) * scale).astype(dtype)
    u2 = (rnd.integers(0, int(1 / scale), 4096) * scale).astype(dtype)
    s, c = ob.oracle_sincos2pi(u2)
    z = T(1.0) - T(2.0) * u1
    r = np.sqrt(T(1.0) - z * z)
    assert_bits(ob.oracle_unit_vec(u1, u2), np.stack([r * c, r * s, z]), "oracle unit_vec")
    v = dm.ref_unit(dm.random_vectors(dtype, 4096, -2, 2, 830))
    n = dm.ref_unit(dm.random_vectors(dtype, 4096, -2, 2, 831))
    ratio = rnd.choice(np.array([1.5, 1 / 1.5, 1.0, 2.4]), 4096).astype(dtype)
    ct = np.minimum((-v[0] * n[0] + -v[1] * n[1]) + -v[2] * n[2], T(1.0))
    rperp = (v + n * ct) * ratio
    rpar = n * -np.sqrt(np.abs(T(1.0) - dm.ref_len2(rperp)))
    assert_bits(ob.oracle_refract(v, n, ratio), rperp + rpar, "oracle refract")


def test_missing_device_library_raises_with_the_make_command(monkeypatch, tmp_path):
    monkeypatch.setattr(du, "_lib", None)
    monkeypatch.setenv("RT_DEVUNIT_LIB", str(tmp_path / "absent.so"))
    with pytest.raises(RuntimeError, match="make -C .* devunit"):
        du.load_devunit()
