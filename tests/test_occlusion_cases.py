"""The launches tests/test_gpu_occlusion.py sends (tests/occlusion_cases.py over tests/query_cases.py's), checked with
the oracle alone so that the GPU test cannot pass vacuously, and the expected bytes checked against a second
reference.  No GPU.

Launch conditions, per launch and mode (the worst found over all 4 scenes x 5 families x 3 kinds x 2 precisions x 2
modes in brackets):
  * under `classes`, at least 1/8 of the valid rays are occluded [0.181] and at least 1/2 are not [0.662];
  * every class holds at least 8 rays that hit [13];
  * in kinds full and mixed, at least 16 batches hold an occluded lane and a valid lane that enters the sweep and
    stays open together [16 and 48]: a done lane beside lanes still walking;
  * under `inf`, in kind full, every family but degenerate has at least 8 batches of 64 valid rays that are all
    occluded [13]: whole waves that leave the sweep early.
"""
import numpy as np
import pytest

import occlusion_cases as oc
import query_cases as qc

N_RESTATE = 192


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("fam", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.SCENES)
def test_launch_conditions(name, fam, kind, prec):
    for mode in qc.MODES:
        la, tm, want = oc.case(name, fam, prec, kind, mode, "classes")
        idx, t = la.ref[mode]
        assert tm.dtype == la.d.dtype and tm.shape == (la.n,) and want.dtype == np.uint8
        cls = oc.classes(la.n)
        hit = idx >= 0
        # the table, class by class, on the rays that hit and on those that do not
        T, inf = tm.dtype.type, tm.dtype.type(np.inf)
        big = np.finfo(tm.dtype).max
        assert np.isinf(tm[cls == 0]).all() and (tm[cls == 0] > 0).all()
        assert np.array_equal(tm[(cls == 1) & hit], t[(cls == 1) & hit]) and (tm[(cls == 1) & ~hit] == big).all()
        assert np.array_equal(tm[(cls == 2) & hit], np.nextafter(t[(cls == 2) & hit], inf)) and np.isinf(tm[(cls == 2) & ~hit]).all()
        assert np.array_equal(tm[(cls == 3) & hit], np.nextafter(t[(cls == 3) & hit], -inf)) and (tm[(cls == 3) & ~hit] == big).all()
        assert np.array_equal(tm[(cls == 4) & hit], T(2) * t[(cls == 4) & hit]) and (tm[(cls == 4) & ~hit] == 1.0).all()
        assert np.array_equal(tm[(cls == 5) & hit], t[(cls == 5) & hit] / T(2)) and (tm[(cls == 5) & ~hit] == 1000.0).all()
        assert (tm[cls == 6] == T(0.001)).all() and (tm[cls == 7] == np.nextafter(T(0.001), T(0))).all()
        r8 = np.flatnonzero(cls == 8)
        assert np.array_equal(tm[r8], np.array([0.0, -1.0, -np.inf], tm.dtype)[r8 % 3])
        assert np.isnan(tm[cls == 9]).all() and not np.isnan(tm[cls != 9]).any()
        # the expected byte, class by class, on the valid rays that hit: only 2 and 4 lie above t
        v = la.valid & hit
        for c, byte in ((0, 1), (1, 0), (2, 1), (3, 0), (4, 1), (5, 0), (6, 0), (7, 0), (8, 0), (9, 255)):
            assert (want[v & (cls == c)] == byte).all(), (mode, c)
        assert (want[~la.valid] == oc.INVALID).all() and (want[la.valid & ~hit & (cls != 9)] == oc.NO).all()
        ok = want != oc.INVALID
        occluded, free = (want[ok] == oc.YES).mean(), (want[ok] == oc.NO).mean()
        per_class = min(int((hit & (cls == c)).sum()) for c in range(oc.N_CLASSES))
        print(name, fam, kind, prec, mode, f"occluded {occluded:.3f}, not {free:.3f}, hits in the emptiest class {per_class}")
        assert occluded >= 1 / 8 and free >= 1 / 2, mode
        assert per_class >= 8, mode
        if kind in ("full", "mixed"):
            stays = (want == oc.NO) & oc.enters(la.valid, tm)
            both = int((oc.batches(want == oc.YES).any(1) & oc.batches(stays).any(1)).sum())
            print("   batches with done and open lanes:", both)
            assert both >= 16, mode
        la, tm, want = oc.case(name, fam, prec, kind, mode, "inf")
        assert np.isinf(tm).all() and (tm > 0).all()
        assert np.array_equal(want[la.valid], (idx[la.valid] >= 0).astype(np.uint8)) and (want[~la.valid] == oc.INVALID).all()
        if kind == "full" and fam != "degenerate":
            whole = int((oc.batches(want) == oc.YES).all(1).sum())
            print("   batches wholly occluded:", whole)
            assert whole >= 8, mode


@pytest.mark.parametrize("prec", qc.PRECS)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("fam", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.SCENES)
def test_second_reference(name, fam, kind, prec):
    """The byte derived from independent_v2.hit_scene's t (query_cases.restate_packed, pure Python) equals the
    oracle-derived one, on up to 192 valid rays of the launch spread over the classes."""
    la, tm, want = oc.case(name, fam, prec, kind, "packed", "classes")
    v = np.flatnonzero(la.valid)
    pick = v[:: max(1, v.size // N_RESTATE)][:N_RESTATE]
    _, t, _, _, _ = qc.restate_packed(la.sc.flat, la.o[pick], la.d[pick], prec)
    again = oc.expected(np.ones(pick.size, bool), t, tm[pick])
    np.testing.assert_array_equal(again, want[pick])
    assert len(set(oc.classes(la.n)[pick].tolist())) == oc.N_CLASSES


def test_expected_is_strict_and_total():
    for dtype in (np.float32, np.float64):
        t = np.array([1.0, 1.0, 1.0, np.inf, np.inf, 2.0, 2.0, np.nan], dtype)
        tm = np.array([1.0, np.nextafter(dtype(1), dtype(2)), np.inf, np.inf, 5.0, np.nan, -np.inf, 3.0], dtype)
        valid = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
        assert oc.expected(valid, t, tm).tolist() == [0, 1, 1, 0, 0, 255, 0, 255]
        assert oc.enters(valid, tm).tolist() == [True, True, True, True, True, False, False, False]
        assert not oc.enters(np.ones(2, bool), np.array([0.001, np.nextafter(dtype(0.001), dtype(0))], dtype)).any()
