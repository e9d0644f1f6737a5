"""Inputs of the fp32 sqrt-form tests (tests/test_gpu_sqrt_forms.py; checked on the CPU by
tests/test_sqrt_forms_cases.py): the named cases the GPU test reports on, and single waves with one lane outside
the short form's range."""
import numpy as np

F32, U32 = np.float32, np.uint32
WAVE = 64
N_CASES = 1 << 20
LO = 0x0F800000            # bits of 2^-96
INF = 0x7F800000
# one argument sqrt_len's short form is not for, per kind: tiny nonzero of either sign, zeros, +inf, NaN, negatives
ODD = np.array([0x00000001, 0x007FFFFF, 0x00800000, LO - 1, 0x80000001, 0x80000000 | (LO - 1), 0x00000000, 0x80000000,
                INF, 0x7FC00000, 0xBF800000, 0xFF800000], U32)


def _bits(a):
    return np.asarray(a, U32).view(F32)


def cases():
    """2^20 fp32 inputs: the first two and last two patterns of every binade from 2^-96 up, exact squares and their
    neighbours one ulp either side, rounded squares of random roots and their neighbours, 2^-96, +-0, +inf, NaN."""
    rng = np.random.default_rng(0x5C11)
    e = np.arange(LO >> 23, 255, dtype=U32) << 23                       # binade starts, 2^-96 .. 2^127 (and inf)
    edges = np.concatenate([e, e + 1, e[1:] - 1, e[1:] - 2])
    # exact squares: a root with a 12-bit significand, any exponent whose square stays in [2^-94, 2^126]
    m = rng.integers(1 << 11, 1 << 12, 150000).astype(np.float64)
    k = rng.integers(-58, 52, m.size)
    sq = np.ldexp(m * m, 2 * k).astype(F32)
    assert (sq.astype(np.float64) == np.ldexp(m * m, 2 * k)).all()
    sq = sq.view(U32)
    special = np.array([LO, 0x00000000, 0x80000000, INF, 0x7FC00000, 0x7F800001, 0xFFFFFFFF], U32)
    fixed = np.concatenate([edges, sq, sq - 1, sq + 1, special])
    # rounded squares of random roots (the root's 24 bits all in use), and their neighbours
    n = (N_CASES - fixed.size) // 3
    r = _bits(rng.integers(0x28000000, 0x5F000000, n, dtype=np.int64))   # 2^-47 .. 2^63
    rs = (r * r).view(U32)
    rest = N_CASES - fixed.size - 3 * n
    pad = rng.integers(LO, INF, rest, dtype=np.int64).astype(U32)
    out = np.concatenate([fixed, rs, rs - 1, rs + 1, pad])
    assert out.size == N_CASES
    return out.view(F32)


def mixed_waves():
    """-> (x, odd): 64 waves per kind of ODD; wave w's lane w % 64 holds the odd argument, the other 63 lanes
    arguments in [2^-96, +inf)."""
    rng = np.random.default_rng(0x5C12)
    waves = ODD.size * WAVE
    x = rng.integers(LO, INF, waves * WAVE, dtype=np.int64).astype(U32).reshape(waves, WAVE)
    odd = np.zeros((waves, WAVE), bool)
    w = np.arange(waves)
    odd[w, w % WAVE] = True
    x[w, w % WAVE] = np.repeat(ODD, WAVE)
    return x.reshape(-1).view(F32), odd.reshape(-1)


def in_range(x):
    """sqrt_len's short-form condition per lane: 2^-96 <= x < +inf."""
    with np.errstate(invalid="ignore"):
        return (x >= F32(2.0 ** -96)) & (x < F32(np.inf))
