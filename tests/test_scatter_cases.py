"""The lanes of tests/scatter_cases.py, checked on the CPU, so that the GPU tests of tests/test_gpu_scatter.py cannot
pass vacuously.  Three things per family, precision and mode:
  * the conditions the family is built for hold, read from the oracle's diagnostics (branch code, front bit, normal);
  * the oracle's next-ray and get-ray probes agree at 0 ulp with a second reference, written per lane from
    tests/independent_v2.py's primitives (every lane of every family: it is fast enough);
  * the same Python function with one thing changed (scatter_cases.MUTANTS) differs from the oracle on at least one
    lane of the family aimed at that change: a kernel wrong in that way could not pass the GPU test.
No device code runs here.  The lane counts per branch code are printed (pytest -s) for the record.
"""
import numpy as np
import pytest

import oracle_bind as ob
import scatter_cases as sc
from device_math_cases import same_bits

PRECS = list(sc.DTYPES)
ALL = pytest.mark.parametrize("mode", sc.MODES)
ALLP = pytest.mark.parametrize("prec", PRECS)
CODE = sc.CODE


def fam(name, prec, mode):
    launches, refs = sc.family(name, prec, mode), sc.family_reference(name, prec, mode)
    for ln in launches:
        la = ln.lanes
        assert la.n % sc.BLOCK == 0 and la.n <= 4096 and la.o.dtype == la.d.dtype == la.c.dtype == sc.DTYPES[prec]
        s = la.role == sc.SCATTER
        assert (la.hit_i[s] >= 0).all() and (la.hit_i[s] < sc.table().n_spheres).all()
        assert (la.sid < (1 << 20)).all() and (la.k[s] < 3839).all()
    return launches, refs


def ulps_apart(a, b):
    u = np.int32 if a.dtype == np.float32 else np.int64
    return np.abs(a.view(u).astype(np.int64) - b.view(u).astype(np.int64))


def test_scene_table():
    f = sc.table()
    assert f.n_spheres == sc.N_S100 + len(sc._SPECIALS) and len(f.materials) == f.n_spheres
    assert (f.material != np.arange(f.n_spheres)).all()          # materials[material[i]], never materials[i]
    assert np.array_equal(f.center[:sc.N_S100], sc.s100().center) and np.array_equal(f.radius[:sc.N_S100], sc.s100().radius)
    for i in range(sc.N_S100):
        assert sc.material_of(i) is sc.s100().materials[sc.s100().material[i]]
    for name, i in sc.SP.items():
        if name != "ground":
            assert sc.material_of(i) is sc._SPECIALS[i - sc.N_S100][3]
    iors = {m.index_of_refraction for m in f.materials if isinstance(m, sc.rt.Dielectric)}
    assert {1.5, 2.4, 1.0003, 1.0, 0.7, 1e-3, 1e3} <= iors
    fuzz = {m.fuzzy_factor for m in f.materials if isinstance(m, sc.rt.Metal)}
    assert {0.0, 1.0, -0.5} <= fuzz
    hit = np.concatenate([ln.lanes.hit_i[ln.lanes.role == sc.SCATTER] for name in sc.FAMILIES
                          for ln in sc.family(name, "f32", "packed")])
    assert 0 in hit and f.n_spheres - 1 in hit


@ALL
@ALLP
@pytest.mark.parametrize("name", sc.FAMILIES)
def test_counts(name, prec, mode):
    """The record: lanes and branch codes per launch."""
    launches, refs = fam(name, prec, mode)
    for ln, ref in zip(launches, refs):
        roles = {r: int((ln.lanes.role == v).sum()) for r, v in (("idle", sc.IDLE), ("camera", sc.CAMERA), ("scatter", sc.SCATTER))}
        print(f"{ln.name} {prec} {mode}: {ln.lanes.n} lanes {roles} {sc.code_counts(ref.code)}")
        assert ((ref.code == sc.NO_CODE) == (ln.lanes.role != sc.SCATTER)).all()


@ALL
@ALLP
def test_ordinary(prec, mode):
    (ln,), (ref,) = fam("ordinary", prec, mode)
    la = ln.lanes
    assert la.n == sc.N_ORDINARY and (la.role == sc.SCATTER).all() and (la.hit_i < sc.N_S100).all()
    counts = sc.code_counts(ref.code)
    assert all(v >= 32 for k, v in counts.items() if k != "near_zero"), counts
    idx, t = ob.oracle_nearest_hit(sc.s100(), mode, la.o, la.d)       # the hits are the reference's own
    own = (idx == la.hit_i) & (t == la.hit_t)
    if mode == "packed":   # ... or, for rays that start inside glass, the ROOT2 mode's
        idx2, t2 = ob.oracle_nearest_hit(sc.s100(), "root2", la.o, la.d)
        own |= (idx2 == la.hit_i) & (t2 == la.hit_t)
    assert own.all()
    d2 = (la.d.astype(np.float64) ** 2).sum(0)
    half = la.n // 2
    assert np.abs(d2[:half] - 1).max() < 1e-5
    assert d2[half:].min() < 1e-5 and d2[half:].max() > 1e5 and 1e-6 * 0.99 <= d2[half:].min() and d2[half:].max() <= 1e6 * 1.01
    assert 0.3 < (np.log10(d2[half:]) < 0).mean() < 0.7
    assert 0 in la.hit_i and (ref.front == 0).sum() >= 32 and (ref.front == 1).sum() >= 32


@ALL
@ALLP
def test_front_bit(prec, mode):
    (ln,), (ref,) = fam("front_bit", prec, mode)
    la, g = ln.lanes, sc.N_FRONT
    plain, fused = ln.tags["plain"], ln.tags["fused"]
    assert la.n == 3 * g and [int(la.hit_i[j * g]) for j in range(3)] == [sc.SP[m] for m in sc.FRONT_MATERIALS]
    kinds = sorted({sc.material_of(i).kind for i in np.unique(la.hit_i)})
    assert kinds == [0, 1, 2]
    eps = np.finfo(la.dtype).eps
    for j in range(3):
        s = slice(j * g, (j + 1) * g)
        assert (np.abs(plain[s].astype(np.float64)) <= 8 * eps).all()      # within a few ulp of the tangent plane
        assert ((plain[s] < 0) != (fused[s] < 0)).sum() >= 64
        assert (plain[s] == 0).sum() >= 64
        used = fused if mode == "packed" else plain
        assert np.array_equal(used[s] < 0, ref.front[s] == 1)
        assert 0.1 < (ref.front[s] == 1).mean() < 0.9
        # the tags are the dots of the lane's direction with the reference's normal before its flip
        normal = ref.nrm[:, s] * np.where(ref.front[s] == 1, 1, -1).astype(la.dtype)
        assert same_bits(sc.plain_dot(la.d[:, s], normal), plain[s]).all()


def pairs_of(la, n_pairs):
    a, b = la.take(np.arange(0, 2 * n_pairs, 2)), la.take(np.arange(1, 2 * n_pairs, 2))
    apart = ulps_apart(a.d, b.d)
    assert (apart.sum(0) == 1).all() and (apart.max(0) == 1).all()       # one component, one ulp
    for f in ("o", "c", "hit_i", "hit_t", "sid", "pix", "k"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    return np.arange(0, 2 * n_pairs, 2), np.arange(1, 2 * n_pairs, 2)


@ALL
@ALLP
def test_tir(prec, mode):
    (ln,), (ref,) = fam("tir", prec, mode)
    la = ln.lanes
    ia, ib = pairs_of(la, ln.tags["pairs"] // 2)
    cannot = ref.code == CODE["cannot_refract"]
    assert (cannot[ia] != cannot[ib]).all()
    assert 0.25 <= cannot.mean() <= 0.75, cannot.mean()
    for name, outward, _ in sc.TIR_CASES:
        at = np.flatnonzero(la.hit_i[:ln.tags["pairs"]] == sc.SP[name])
        assert at.size >= 16 and (ref.front[at] == (0 if outward else 1)).all(), name
        assert cannot[at].any() and not cannot[at].all()
    # the lanes at which ratio * sin(theta) is exactly 1 do refract
    eq = np.arange(ln.tags["pairs"], ln.tags["n"])
    _, prod = sc.sin_product(la, ref)
    assert eq.size >= 1 and (prod[eq] == 1).all() and not cannot[eq].any()
    # and the pairs straddle the comparison as computed from the diagnostics
    assert ((prod[:ln.tags["pairs"]] > 1) == cannot[:ln.tags["pairs"]]).all()


@ALL
@ALLP
def test_schlick(prec, mode):
    (ln,), (ref,) = fam("schlick", prec, mode)
    la = ln.lanes
    n_pairs = ln.tags["n"] // 2
    assert n_pairs >= 64
    ia, ib = pairs_of(la, n_pairs)
    refl = ref.code == CODE["schlick_reflect"]
    assert set(np.unique(ref.code[:2 * n_pairs])) == {CODE["schlick_reflect"], CODE["refract"]}
    assert (refl[ia] != refl[ib]).all()
    for name, outward in sc.SCHLICK_CASES:
        at = np.flatnonzero(la.hit_i[:2 * n_pairs] == sc.SP[name])
        assert at.size >= 64 and (ref.front[at] == (0 if outward else 1)).all(), name     # r0_back : r0_front
        assert sc.material_of(sc.SP[name]).index_of_refraction not in (1.0, 1.5)
    _, ua, ub = ob.oracle_draw(la.dtype, la.sid, la.pix, la.k, np.full(la.n, 2), sc.SEED)
    assert (ua > 0.03).all() and (ua < 0.98).all() and (np.abs(ua - ub) > 1e-3).mean() > 0.9


@ALL
@ALLP
def test_clamp(prec, mode):
    (ln,), (ref,) = fam("clamp", prec, mode)
    la, T = ln.lanes, sc.DTYPES[prec]
    raw = sc.cos_theta(la, ref)
    assert not np.isnan(raw).any()
    one = T(1)
    below, above = np.nextafter(one, T(0)), np.nextafter(one, T(2))
    for v in (one, below, above, T(2), T(1e3), -one, -below, -above, T(-2), T(-1e3)):
        assert (raw == v).sum() >= 6, v                # along the six axes the normal is exact
    with np.errstate(all="ignore"):
        arg, prod = sc.sin_product(la, ref)
    # sqrt_nd's contract: its argument is 0, or at least 2^-24 (2^-53) in magnitude
    floor = 2.0 ** (-24 if prec == "f32" else -53)
    assert ((arg == 0) | (np.abs(arg.astype(np.float64)) >= floor)).all()
    assert (arg == 0).sum() >= 24 and (arg < 0).sum() >= 24 and ((arg > 0) & (arg < 1e-6)).sum() >= 6
    neg = raw < -1
    assert np.isnan(prod[neg]).all() and (ref.code[neg] == CODE["schlick_reflect"]).all()     # sin NaN, cannot false, Schlick > 1
    hollow = np.array([sc.material_of(i).hollow for i in la.hit_i])
    assert hollow[neg].all() and (ref.front == 0).sum() > 100 and (ref.front == 1).sum() > 100


@ALL
@ALLP
def test_near_zero(prec, mode):
    (ln,), (ref,) = fam("near_zero", prec, mode)
    la, n, pert = ln.lanes, ln.tags["n"], ln.tags["perturbed"]
    code = ref.code[:n]
    exact = ~pert
    assert (code[exact] == CODE["near_zero"]).sum() >= 256
    if prec == "f64" or mode == "scalar":
        assert (code[exact] == CODE["near_zero"]).all()
    else:   # fp32, packed: only where the normal's length rounds to 1
        assert 0.6 < (code[exact] == CODE["near_zero"]).mean() < 0.9
    # a near-zero lane leaves along its normal (-rv = -d here, where the normal's length is exactly 1)
    nz = np.flatnonzero(exact & (code == CODE["near_zero"]))
    assert same_bits(ref.d[:, nz], ref.nrm[:, nz]).all()
    assert same_bits(ref.d[:, nz], -la.d[:, nz]).all(0).mean() > 0.6
    # perturbed lanes: both sides of 1e-8
    assert (code[pert] == CODE["near_zero"]).sum() >= 32 and (code[pert] == CODE["lambertian"]).sum() >= 32
    away = np.flatnonzero(pert & (code == CODE["lambertian"]))
    mag = np.abs(ref.d[:, away].astype(np.float64)).max(0)
    assert (mag >= 1e-8).all() and (mag < 1e-7).sum() >= 8           # just above: a threshold of 1e-7 would take them
    radii = {float(sc.table().radius[i]) for i in np.unique(la.hit_i)}
    assert radii == ({1.0, -1.0} if mode == "scalar" else {1.0})


@ALL
@ALLP
def test_colour(prec, mode):
    (ln,), (ref,) = fam("colour", prec, mode)
    la, n = ln.lanes, ln.tags["n"]
    fi = np.finfo(la.dtype)
    cin, cout = la.c[:, :n], ref.c[:, :n]
    sub_in = (cin != 0) & (np.abs(cin) < fi.tiny)
    assert (cin == 0).any() and (np.signbit(cin) & (cin == 0)).any() and sub_in.any()
    sub_out = (cout != 0) & (np.abs(cout) < fi.tiny)
    assert (sub_out & ~sub_in).sum() >= 3          # a normal colour times an albedo below 1: a subnormal
    assert ((cout == 0) & (cin != 0)).sum() >= 3    # ... and products that round to 0
    glass = np.array([sc.material_of(i).kind == 2 for i in la.hit_i[:n]])
    assert glass.sum() >= 32 and same_bits(cout[:, glass], cin[:, glass]).all()
    mats = [sc.material_of(i) for i in np.unique(la.hit_i)]
    assert {m.albedo for m in mats if m.kind == 0} >= {(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)}
    assert {m.fuzzy_factor for m in mats if m.kind == 1} >= {0.0, 1.0, -0.5}


@ALL
@ALLP
def test_scalar_normals(prec, mode):
    (ln,), (ref,) = fam("scalar_normals", prec, mode)
    la, special = ln.lanes, ln.tags["special"]
    per_wave = special.reshape(-1, sc.WAVE).sum(1)
    assert (per_wave == 32).all()                                           # every wave: half and half
    f = sc.table()
    r = f.radius[la.hit_i[special]]
    assert {1000.0, 1e-3, -0.2, -1.0, -1000.0} <= set(r.tolist())
    assert (la.hit_i[~special] < sc.N_S100).all()
    if mode == "scalar":
        # the normal is (p - c) / radius: not of length 1, and against p - c for a negative radius
        s = np.flatnonzero(special)
        ln2 = (ref.nrm[:, s].astype(np.float64) ** 2).sum(0)
        assert (ln2 != 1).mean() > 0.5 and np.abs(ln2 - 1).max() < 1e-2
        vec = ref.o[:, s].astype(np.float64) - f.center[la.hit_i[s]].T
        outward = (vec * ref.nrm[:, s]).sum(0) * np.where(ref.front[s] == 1, 1, -1)
        assert ((outward < 0) == (r < 0)).all()
        assert (ref.front[s] == 1).sum() > 50 and (ref.front[s] == 0).sum() > 50


@ALL
@ALLP
def test_camera(prec, mode):
    launches, refs = fam("camera", prec, mode)
    dtype = sc.DTYPES[prec]
    assert [ln.cam_name for ln in launches] == ["main", "defocus", "one", "minus_zero"]
    flags = {ln.cam_name: sc.host_pinhole(ln.cam, dtype) for ln in launches}
    assert flags == {"main": True, "defocus": False, "one": True, "minus_zero": False}
    assert any(v == 0 and np.signbit(v) for v in launches[3].cam.center) and all(v == 0 for v in launches[3].cam.du)
    for ln, ref in zip(launches, refs):
        la, cam = ln.lanes, ln.cam
        W, H = cam.image_width, cam.image_height
        assert (la.role == sc.CAMERA).all()
        seen = set(zip(la.pix.tolist(), la.sid.tolist()))
        assert seen == {(p, s) for p in range(W * H) for s in range(16)}
        assert np.array_equal(la.pix, la.rowy * W + la.colx) and (la.colx < W).all() and (la.rowy < H).all()
        assert np.abs((ref.d.astype(np.float64) ** 2).sum(0) - 1).max() < 1e-5 and (ref.c == 1).all()
    assert (W, H) == (8, 5) and [(ln.cam.image_width, ln.cam.image_height) for ln in launches[:3]] == [(16, 9), (7, 5), (1, 1)]
    # the defocus camera's rejection loop diverges: some lanes take the first try, others do not
    la = launches[1].lanes
    _, ua, ub = ob.oracle_draw(dtype, la.sid, la.pix, np.zeros(la.n), np.ones(la.n), sc.SEED)
    x, y = dtype(2) * ua - dtype(1), dtype(2) * ub - dtype(1)
    first = x * x + y * y <= 1
    assert 0.1 < (~first).mean() < 0.4 and (~first).reshape(-1, sc.WAVE).any(1).all()
    assert np.unique(refs[1].o, axis=1).shape[1] > 500 and np.unique(refs[0].o, axis=1).shape[1] == 1


@ALL
@ALLP
def test_mixed(prec, mode):
    (roles, lane7), (ref, ref7) = fam("mixed", prec, mode)
    r = roles.lanes.role.reshape(-1, sc.WAVE)
    cam, sca, idle = (r == sc.CAMERA).sum(1), (r == sc.SCATTER).sum(1), (r == sc.IDLE).sum(1)
    full, half = idle == 0, idle == 32
    assert (full | half).all()
    for rows, size in ((full, 64), (half, 32)):
        have = set(zip(cam[rows].tolist(), sca[rows].tolist()))
        if size == 64:
            assert {(0, 64), (64, 0), (32, 32), (1, 63), (63, 1)} <= have, have
        else:
            assert any(c == 0 for c, s in have) and any(s == 0 for c, s in have) and any(c > 0 and s > 0 for c, s in have), have
    alternating = (r[:, 0::2] == sc.SCATTER).all(1) & (r[:, 1::2] == sc.CAMERA).all(1)
    assert alternating.sum() == 4
    un = roles.lanes.role == sc.IDLE
    assert (roles.lanes.o[:, un] == sc.UNTOUCHED).all() and same_bits(ref.o[:, un], roles.lanes.o[:, un]).all()
    # the second launch: lane 7 of every odd wave has a tiny, nonzero |hit - centre|^2
    la, tiny = lane7.lanes, lane7.tags["tiny"]
    assert np.array_equal(np.flatnonzero(tiny), np.arange(1, la.n // sc.WAVE, 2) * sc.WAVE + 7)
    vec2 = ((ref7.o[:, tiny].astype(np.float64) - sc.table().center[la.hit_i[tiny]].T) ** 2).sum(0)
    assert (vec2 > 0).all() and (vec2 < 2.0 ** -96).all()
    assert np.isfinite(ref7.d[:, tiny]).all()


# ---------------------------------------------------------------- the second reference
def differs(ln, ref, mode, idx, mutate=None):
    """Per listed lane: does the Python reference (with the mutation) differ from the oracle in any bit of o, d, c?"""
    o, d, c = sc.lanes_py(ln.lanes, idx, mode, ln.cam, mutate)
    return ~(same_bits(o, ref.o[:, idx]).all(0) & same_bits(d, ref.d[:, idx]).all(0) & same_bits(c, ref.c[:, idx]).all(0))


@ALL
@ALLP
@pytest.mark.parametrize("name", sc.FAMILIES)
def test_oracle_against_python(name, prec, mode):
    launches, refs = fam(name, prec, mode)
    for ln, ref in zip(launches, refs):
        idx = np.arange(ln.lanes.n)
        if "tiny" in ln.tags and prec == "f32":
            idx = idx[~ln.tags["tiny"]]     # independent_v2's exact fp32 fma does not model subnormal results
        bad = differs(ln, ref, mode, idx)
        assert not bad.any(), (ln.name, int(bad.sum()), idx[bad][:8].tolist())


MUTANT_FAMILY = {"plain_front": "front_bit", "unflipped": "front_bit", "cannot_ge": "tir", "schlick_ub": "schlick",
                 "r0_swapped": "schlick", "no_hollow": "clamp", "near_1e-7": "near_zero", "near_1e-9": "near_zero",
                 "abs_radius": "scalar_normals"}
MUTANT_MODES = {"plain_front": ("packed",), "abs_radius": ("scalar",)}     # what the other mode does not have


def test_every_mutant_has_a_family():
    assert set(MUTANT_FAMILY) == set(sc.MUTANTS)


@ALL
@ALLP
@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_mutant_is_caught(mutant, prec, mode):
    if mode not in MUTANT_MODES.get(mutant, sc.MODES):
        # the mutation changes nothing this mode runs: the Python function must then still agree
        (ln, *_), (ref, *_) = fam(MUTANT_FAMILY[mutant], prec, mode)
        assert not differs(ln, ref, mode, np.arange(ln.lanes.n), mutant).any()
        return
    (ln, *_), (ref, *_) = fam(MUTANT_FAMILY[mutant], prec, mode)
    idx = np.arange(ln.lanes.n)
    assert not differs(ln, ref, mode, idx).any()
    caught = differs(ln, ref, mode, idx, mutant)
    print(f"{mutant} {prec} {mode}: caught on {int(caught.sum())} of {idx.size} lanes of {ln.name}")
    assert caught.any()
