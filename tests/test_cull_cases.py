"""The adversarial rays of tests/cull_cases.py, checked on the CPU with the oracle alone, so that the GPU tests
of tests/test_gpu_cull_probe.py cannot pass vacuously: the scenes have the structure each is meant to reach
(build_scene_image's counts), and per (scene, family, mode, precision) the reference itself accepts, rejects and
reports the targets in the stated shares, a stated share of the accepted ones lying outside the sphere by less than
the reference's own rounding.  The numbers are conditions on the inputs; no device code runs here.
"""
import numpy as np
import pytest

import cull_cases as cc

SCENE_NAMES = list(cc.SCENES)
TARGET_FAMILIES = ("graze", "box_graze") + cc.CAMERA_FAMILIES
# the measured delta below which an accepted ray outside its sphere is a hit the reference owes to its own rounding
OUTSIDE = {"f32": 1e-6, "f64": 1e-13}


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_structure(name):
    sc = cc.scene(name)
    want = cc.SCENES[name][1]
    assert {k: sc.counts[k] for k in want} == want, sc.counts
    assert sc.counts["n_xg"] == (1 if sc.counts["n_xs"] else 0)
    n = sc.flat.n_spheres
    assert sorted(sc.ridx[sc.ridx != 0xFFFFFFFF].tolist()) == list(range(n))
    clusters = sc.clusters()
    assert sum(len(c) for c in clusters) == n - sc.counts["n_xs"] and max(len(c) for c in clusters) <= 16
    if name == "d_mega_far":   # the same spheres as d_mega, 1e3 .. 1e4 extents away
        near = cc.scene("d_mega")
        shift = sc.flat.center - near.flat.center
        assert np.array_equal(sc.flat.radius, near.flat.radius) and np.abs(shift - shift[0]).max() < 1e-6
        assert 1e3 <= np.linalg.norm(shift[0]) / (2 * near.half) <= 1e4


@pytest.mark.parametrize("prec", list(cc.DTYPES))
@pytest.mark.parametrize("fam", TARGET_FAMILIES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_shares(name, fam, prec):
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    rays = cc.family(sc, fam, dtype)
    assert rays.n == cc.N_CASES and (rays.target >= sc.first).all() and np.isfinite(rays.delta).all()
    assert rays.o.dtype == rays.d.dtype == dtype
    # the construction: both signs, the whole delta range, near and far origins, unit and other lengths
    ad = np.abs(rays.delta)
    assert (rays.delta > 0).mean() > 0.3 and (rays.delta < 0).mean() > 0.25
    assert (ad < 1e-3).mean() > 0.7 and np.median(ad) < 3e-5
    dl = np.sqrt((rays.d.astype(np.float64) ** 2).sum(0))
    assert dl.min() < 1e-2 and dl.max() > 1e2 and (np.abs(dl - 1) < 1e-3).mean() > 0.3
    outside = (rays.delta > 0) & (rays.delta < OUTSIDE[prec])
    for mode in cc.MODES:
        acc = cc.accepts(sc, mode, rays)
        idx, _ = cc.reference(sc, mode, rays)
        shares = dict(accept=acc.mean(), reject=(~acc).mean(), nearest=(idx == rays.target).mean(),
                      owed=(acc & outside).sum() / max(1, acc.sum()))
        print(name, fam, prec, mode, {k: round(float(v), 3) for k, v in shares.items()})
        assert shares["accept"] >= 0.30, (mode, shares)
        assert shares["reject"] >= 0.30, (mode, shares)
        assert shares["nearest"] >= 0.20, (mode, shares)
        assert shares["owed"] >= 0.10, (mode, shares)
        # the solo and bundle compositions take the first N_SOLO cases: the same shares hold there
        h = slice(0, cc.N_SOLO)
        assert acc[h].mean() >= 0.30 and (~acc[h]).mean() >= 0.30 and (idx[h] == rays.target[h]).mean() >= 0.20, mode


@pytest.mark.parametrize("prec", list(cc.DTYPES))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_box_graze_touches_the_box_face(name, prec):
    """The target sets its cluster's extent on the ray's axis, and the ray runs along that face: its component on
    the axis is one of the clamp values exactly, or a tilt of at most 1e-3 plus the rounded origin's (below 1e-3)."""
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    rays = cc.box_graze(sc, dtype)
    C, r = sc.geom(dtype)
    member = {int(j): m for m in sc.clusters() for j in m}
    d = rays.d.astype(np.float64)
    ax, cols = rays.axis, np.arange(rays.n)
    da = d[ax, cols]
    assert (np.abs(da) / np.sqrt((d * d).sum(0)) <= 2.1e-3).all()
    clamp = {float(dtype(v)) for v in cc.CLAMP_VALUES}
    exact = np.array([float(v) in clamp for v in da])
    assert 0.15 < exact.mean() < 0.5
    for v in cc.CLAMP_VALUES:   # every signed clamp value occurs
        assert ((da == float(dtype(v))) & (np.signbit(da) == np.signbit(v))).any(), v
    assert ((d == 0).sum(0) == 2).mean() > 0.005 and (np.abs(da[~exact]) > 1e-4 * np.sqrt((d * d).sum(0))[~exact]).any()
    for i in range(rays.n):
        j, a = int(rays.target[i]), int(ax[i])
        m = member[j]
        m = m[m >= sc.first]
        hi, lo = (C[a, m] + r[m]).max(), (C[a, m] - r[m]).min()
        assert C[a, j] + r[j] == hi or C[a, j] - r[j] == lo


@pytest.mark.parametrize("prec", list(cc.DTYPES))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_near_equal_roots(name, prec):
    """Two spheres of different clusters (different supers where the scene has several) whose valid roots differ by
    0, +1 and -1 ulp, in every mode; the nearest hit is mostly one of the two, so the bound and the tie rule decide."""
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    cl = sc.cluster_of()
    assert len(sc.pairs) >= 2
    for a, b in sc.pairs:
        assert cl[a] >= 0 and cl[b] >= 0 and cl[a] != cl[b]
        if sc.counts["n_top"] > 1:
            assert cl[a] // 4 != cl[b] // 4
    rays = cc.near_equal(sc, dtype)
    assert rays.n == cc.N_CASES and np.unique(rays.pair).size >= 2
    for mode in cc.MODES:
        ulps = np.full(rays.n, 1 << 40)
        valid = np.zeros(rays.n, bool)
        for pi, (a, b) in enumerate(sc.pairs):
            m = np.flatnonzero(rays.pair == pi)
            if m.size:
                valid[m], ulps[m] = cc.root_pair(sc, mode, rays.take(m), a, b)
        ulps = ulps[valid]
        print(name, prec, mode, {k: int((ulps == k).sum()) for k in range(-4, 5)}, round(float(valid.mean()), 3))
        assert valid.mean() > 0.9
        for k in (0, 1, -1):
            assert (ulps == k).sum() >= 4, (mode, k)
        assert (np.abs(ulps) >= 2).sum() >= 4 and (np.abs(ulps) <= 4).mean() > 0.3
        idx, _ = cc.reference(sc, mode, rays)
        ab = np.array(sc.pairs)[rays.pair]
        assert ((idx == ab[:, 0]) | (idx == ab[:, 1])).mean() > 0.5, mode
        for k in (0, 1, -1):   # the solo composition's cases
            assert (ulps[:cc.N_SOLO] == k).any(), (mode, k)


@pytest.mark.parametrize("prec", list(cc.DTYPES))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_degenerate_family(name, prec):
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    rays = cc.degenerate(sc, dtype)
    o, d = rays.o.astype(np.float64), rays.d.astype(np.float64)
    L = d[0] * d[0] + d[2] * d[2]
    assert ((L < 1e-15) & (np.abs(d[1]) == 1)).mean() > 0.3          # the filter's zero basis: L < 1e-15
    assert (np.abs(o).sum(0) > 1e14).mean() > 0.3                     # |o|_1 around 1e15
    assert ((d == 0).sum(0) >= 1).mean() > 0.3 and ((d == 0).sum(0) == 2).mean() > 0.1
    assert np.isfinite(o).all() and np.isfinite(d).all() and ((d * d).sum(0) > 0).all()
    idx, _ = cc.reference(sc, "packed", rays)
    assert 0.2 < (idx >= 0).mean()                                    # they are aimed at spheres: many hit


@pytest.mark.parametrize("prec", list(cc.DTYPES))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_camera_centres(name, prec):
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    C, r = sc.geom(dtype)
    eps = float(np.finfo(dtype).eps)
    for which in cc.CENTRES:
        P, j, cand = cc.camera_centre(sc, dtype, which)
        assert P.dtype == dtype and cand.size >= (6 if which == "inside" else 8)
        w = P.astype(cc.LD)[:, None] - C
        inside = set(np.flatnonzero((w * w).sum(0) <= r * r).tolist())
        if which.startswith("outside"):
            assert inside == set()
        elif which == "inside":
            assert inside == {cc.SHELL} and j == cc.SHELL
            assert set(cand.tolist()) <= set(range(cc.SHELL + 1, cc.SHELL + 1 + cc.N_INNER))
        else:   # on: the reference's own c, in the ray type, is <= 0, and no further below than the type's grid at P puts it
            c = cc.ref_c(P - C[:, j].astype(dtype), dtype(r[j]) * dtype(r[j]))
            assert c <= 0 and abs(float(c)) <= 16 * eps * float(r[j]) * (float(np.abs(P).max()) + float(r[j]))
            assert inside <= {j}
        rays = cc.camera(sc, dtype, which)
        assert (rays.o == P[:, None]).all() and set(rays.target.tolist()) <= set(cand.tolist())
        k = np.sqrt(((C[:, rays.target] - P.astype(cc.LD)[:, None]) ** 2).sum(0)) / r[rays.target]
        assert k.max() <= 15 and k.min() >= 1.05


@pytest.mark.parametrize("prec", list(cc.DTYPES))
@pytest.mark.parametrize("name", ["a_one_super", "d_mega_far"])
def test_compositions(name, prec):
    sc, dtype = cc.scene(name), cc.DTYPES[prec]
    for fam, kinds in (("graze", cc.COMPOSITIONS), ("camera:outside_0", cc.CAMERA_COMPOSITIONS)):
        rays = cc.family(sc, fam, dtype)
        for kind in kinds:
            la = cc.compose(sc, fam, dtype, kind)
            n = la.rays.n
            assert n % 256 == 0 and n <= cc.MAX_RAYS and la.active.shape == (n,)
            waves = la.active.reshape(-1, 64)
            has = la.lane_case >= 0
            assert np.array_equal(la.rays.d[:, has & (kind != "bundle")], rays.d[:, la.lane_case[has & (kind != "bundle")]])
            if kind == "solo":
                assert (waves.sum(1) == 1).all()
                assert [int(w.argmax()) for w in waves[:8]] == list(cc.SOLO_LANES) * 2
                assert np.array_equal(la.lane_case[la.active == 1], np.arange(cc.N_SOLO))
            else:
                assert la.active.all()
            if kind == "full":
                assert sorted(la.lane_case.tolist()) == list(range(rays.n))
            if kind == "mixed":   # case, degenerate lane, missing lane, in turn
                assert (la.lane_case[0::3] >= 0).all() and (la.lane_case[1::3] < 0).all() and (la.lane_case[2::3] < 0).all()
                idx, _ = cc.reference(sc, "root2", la.rays)
                assert (idx[2::3] == -1).mean() > (0.5 if fam.startswith("camera") else 0.99)   # from inside the scene some hit
            d = la.rays.d.astype(np.float64)
            u = (d / np.sqrt((d * d).sum(0))).T.reshape(-1, 64, 3)
            cos = (u * u[:, :1]).sum(-1).min(1)   # against the first lane, the camera cone's axis
            if fam.startswith("camera") and kind == "bundle":
                assert (cos > 1 - 1e-8).all()
                assert (la.rays.target >= 0).all() and np.isfinite(la.rays.delta).all()
            if fam.startswith("camera") and kind == "full":
                assert (cos < 0.5).all()          # a spread beyond 60 degrees: camera_sweep's `all`
