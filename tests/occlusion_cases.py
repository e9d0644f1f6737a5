"""Occlusion queries (rt_query_occluded_async): the t_max assignments and expected bytes that
tests/test_occlusion_cases.py (CPU: the launches checked with the oracle alone) and tests/test_gpu_occlusion.py (GPU:
occlusion_rays<T, ROOT2, MEGA> against them) share.

Plain module: no GPU, no fixtures.  The launches are tests/query_cases.py's, unchanged: launch(name, fam, prec, kind)
with its oracle references la.ref[mode] = (index, t).  The oracle for a byte is the header's equivalence: a ray is
occluded iff the closest hit of rt_query_hits_async exists and its t < t_max, strictly; a ray outside the query's
precondition, or with a NaN t_max, is RT_OCCLUDED_INVALID.

Two t_max assignments per launch and mode:
  inf      every ray has +inf.
  classes  cls = default_rng(la.n).integers(0, 10, la.n) picks a class per ray; t is the reference closest hit of the
           ray under the mode, max the largest finite value of the ray type, and a ray that misses (or is invalid: its
           reference t is NaN) takes the substitute in brackets:
             0  +inf                            5  t / 2  [1000.0]
             1  t                   [max]       6  T(0.001)
             2  nextafter(t, +inf)  [+inf]      7  nextafter(T(0.001), 0)
             3  nextafter(t, -inf)  [max]       8  0, -1, -inf by ray % 3
             4  2 t                 [1.0]       9  NaN
"""
import functools

import numpy as np

import cull_cases as cc
import query_cases as qc
from rt_mi355x import abi

ASSIGNMENTS = ("inf", "classes")
N_CLASSES = 10
NO, YES, INVALID = abi.RT_OCCLUDED_NO, abi.RT_OCCLUDED_YES, abi.RT_OCCLUDED_INVALID


def classes(n):
    """The class of each of n rays."""
    return np.random.default_rng(n).integers(0, N_CLASSES, n)


def assign(index, t, how):
    """t_max [n] in t's type for the reference closest hits (index, t) under assignment `how`."""
    dtype = t.dtype
    T = dtype.type
    n = t.shape[0]
    if how == "inf":
        return np.full(n, np.inf, dtype)
    assert how == "classes"
    cls = classes(n)
    hit = np.asarray(index) >= 0
    big, inf = np.finfo(dtype).max, T(np.inf)
    th = np.where(hit, t, T(1.0)).astype(dtype)   # a finite stand-in where there is no hit (replaced below)
    with np.errstate(over="ignore"):
        table = [
            np.full(n, inf, dtype),
            np.where(hit, th, big),
            np.where(hit, np.nextafter(th, inf), inf),
            np.where(hit, np.nextafter(th, -inf), big),
            np.where(hit, T(2.0) * th, T(1.0)),
            np.where(hit, th / T(2.0), T(1000.0)),
            np.full(n, T(0.001), dtype),
            np.full(n, np.nextafter(T(0.001), T(0.0)), dtype),
            np.array([0.0, -1.0, -np.inf], dtype)[np.arange(n) % 3],
            np.full(n, np.nan, dtype),
        ]
    out = np.choose(cls, [a.astype(dtype) for a in table]).astype(dtype)
    return out


def expected(valid, t, t_max):
    """The byte per ray: 255 where the ray is invalid or its t_max is NaN, else (reference closest t) < t_max; a
    miss's reference t is +inf, which is below no bound."""
    with np.errstate(invalid="ignore"):
        occ = np.asarray(t) < np.asarray(t_max)
    return np.where(~np.asarray(valid, bool) | np.isnan(t_max), INVALID, np.where(occ, YES, NO)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name, fam, prec, kind, mode, how):
    """(launch, t_max [n], expected bytes [n]) of one launch, mode and assignment; computed once, read-only."""
    la = qc.launch(name, fam, prec, kind)
    idx, t = la.ref[mode]
    tm = assign(idx, t, how)
    want = expected(la.valid, t, tm)
    tm.setflags(write=False)
    want.setflags(write=False)
    return la, tm, want


def enters(valid, t_max):
    """The rays that enter the sweep: valid, with t_max above T(0.001) (NaN compares false)."""
    t_max = np.asarray(t_max)
    with np.errstate(invalid="ignore"):
        return np.asarray(valid, bool) & (t_max > t_max.dtype.type(0.001))


def batches(a):
    """A per-ray array as [batches, 64] (every launch is whole waves)."""
    return np.asarray(a).reshape(-1, cc.WAVE)


# ---------------------------------------------------------------- the early exit's rays
def ground_rays(sc, dtype, n=128):
    """n rays from inside the scene's box, downwards within about 25 degrees of -y: each meets the ground sphere
    (scene index 0, the scene's one always-exact sphere) from outside, whatever else lies on its way.
    Returns (o [n, 3], d [n, 3])."""
    rng = np.random.default_rng(n)
    half = sc.half
    o = sc.mid[None, :] + rng.uniform(-0.8 * half, 0.8 * half, (n, 3))
    d = np.stack([rng.uniform(-0.4, 0.4, n), -np.ones(n), rng.uniform(-0.4, 0.4, n)], 1)
    d *= rng.uniform(0.5, 2.0, (n, 1))
    return np.ascontiguousarray(o, dtype=dtype), np.ascontiguousarray(d, dtype=dtype)
