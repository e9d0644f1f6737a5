"""tests/step_cases.py checked with the oracle alone, so that the GPU tests' expectations are proven without a GPU:
the loop of steps (oracle_nearest_hit + oracle_next_ray + integrators.sky, reduced by integrators.reduce_samples)
equals oracle_render in mode "vectorized" bit for bit, no lane of it violates the query's precondition, and
integrators.sky is the oracle's sky."""
import numpy as np
import pytest

import oracle_bind as ob
import scatter_cases as sc
import step_cases as stc
from query_cases import assert_same
from rt_mi355x import abi, integrators


@pytest.mark.parametrize("prec", stc.PRECS)
@pytest.mark.parametrize("mode", stc.MODES)
@pytest.mark.parametrize("spp", stc.SPPS)
def test_the_loop_of_steps_is_a_vectorized_render(prec, mode, spp):
    res = stc.loop(prec, mode, spp)
    lin, segs = stc.render(prec, mode, spp)
    assert res.invalid == 0, "a lane left the query's |d|^2 range: choose another scene or seed"
    assert_same(integrators.reduce_samples(res.radiance, stc.W * stc.H, spp), lin, f"linear {prec} {mode} spp {spp}")
    assert res.segments == segs
    assert res.radiance.dtype == stc.DTYPES[prec] and res.radiance.any()


@pytest.mark.parametrize("prec", stc.PRECS)
def test_the_long_loop_is_a_vectorized_render(prec):
    bounces, spp = stc.LONG
    res = stc.loop(prec, "packed", spp, bounces)
    lin, segs = stc.render(prec, "packed", spp, bounces)
    assert res.invalid == 0
    assert_same(integrators.reduce_samples(res.radiance, stc.W * stc.H, spp), lin, "linear")
    assert res.segments == segs


def test_the_loop_cannot_pass_vacuously():
    """The images differ between the modes and the precisions, paths end by all three rules (a miss at bounce 0, a miss
    later, alive at the end), and a loop with one thing changed no longer equals the render."""
    a, _ = stc.render("f64", "packed", 4)
    b, _ = stc.render("f64", "root2", 4)
    c, _ = stc.render("f32", "packed", 4)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    res = stc.cpu_loop("f64", "packed", 4, stc.BOUNCES, keep_steps=True)
    first = res.steps[0][0]
    assert (first == abi.RT_STEP_MISSED).any() and (first == abi.RT_STEP_SCATTERED).any()
    last = res.steps[-1][0]
    assert (last == abi.RT_STEP_SCATTERED).any(), "no path is still alive after the last step"
    assert any((s[0] == abi.RT_STEP_MISSED).any() for s in res.steps[1:])
    # the sky of the primary direction (quirk Q2 of the live path) is another image
    o, d, pix, sid = stc.primary_rays("f64", 4)
    wrong = res.radiance.copy()
    gone = np.flatnonzero(res.radiance.any(1))
    later = gone[res.steps[0][0][gone] == abi.RT_STEP_SCATTERED]
    assert later.size
    colour = res.steps[-1][3]
    wrong[later] = colour[later] * integrators.sky(d[later, 1])
    assert not np.array_equal(integrators.reduce_samples(wrong, stc.W * stc.H, 4), a)
    # and so is a plain sum over the samples in order (6 spp: a partial chunk)
    r6 = stc.loop("f32", "packed", 6).radiance.reshape(stc.W * stc.H, 6, 3)
    acc = np.zeros((stc.W * stc.H, 3), np.float32)
    for s in range(6):
        acc = acc + r6[:, s]
    assert not np.array_equal((acc / np.float32(6)).astype(np.float64), stc.render("f32", "packed", 6)[0])


@pytest.mark.parametrize("prec", stc.PRECS)
def test_the_light_inside_the_ground_reaches_no_hit(prec):
    """What tests/test_gpu_path_step.py expects of direct_light, judged with the oracle: with the light inside the
    ground sphere no hit of the loop is lit; the light in the open reaches many."""
    assert stc.lit_lanes(prec, stc.LIGHT_INSIDE) == (0, stc.lit_lanes(prec, stc.LIGHT_OPEN)[1])
    lit, rays = stc.lit_lanes(prec, stc.LIGHT_OPEN)
    assert rays > 0 and lit > rays // 5


@pytest.mark.parametrize("prec", stc.PRECS)
def test_sky_is_the_oracles_sky(prec):
    """integrators.sky against the oracle's sky, observed through a render of the empty scene in mode "vectorized":
    every primary ray misses at bounce 0, so at 1 spp a pixel is (((0 + sky) + 0) + 0 + 0) / 1 = sky(d.y) exactly."""
    import rt_mi355x as rt
    dtype = stc.DTYPES[prec]
    empty = rt.FlatScene(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.uint32), [rt.Lambertian((0.5, 0.5, 0.5))])
    cam = rt.camera_new_py(24, 40, **dict(rt.MAIN_CAMERA, view_angle=150.0))
    _, lin, _, rc = ob.oracle_render(empty, cam, 4, 1, stc.SEED, flags=stc.V1, precision=prec)
    pix = np.arange(24 * 40, dtype=np.uint32)
    _, d = ob.oracle_get_ray(dtype, cam, stc.SEED, pix % 24, pix // 24, pix, np.zeros_like(pix))
    got = integrators.sky(d[1])
    assert got.dtype == dtype and got.shape == (pix.size, 3)
    assert_same(got.astype(np.float64), lin, "sky over a frame of directions")
    assert d[1].min() < -0.5 and d[1].max() > 0.5
    # edge values: the operations in the oracle's order, every one rounded once (oracle_impl.h sky)
    t = dtype
    fi = np.finfo(dtype)
    ys = np.array([0.0, -0.0, 1.0, -1.0, fi.tiny, -fi.tiny, fi.smallest_subnormal, 1e-9, -1e-9, np.nextafter(t(1), t(0)),
                   np.nextafter(t(-1), t(0)), 0.5, 1 / 3, 1000.0, -1000.0, fi.max, -fi.max, np.inf, -np.inf, np.nan], dtype)
    got = integrators.sky(ys)
    with np.errstate(all="ignore"):
        for i, y in enumerate(ys):
            a = t(t(y + t(1.0)) * t(0.5))
            oma = t(-a + t(1.0))
            want = np.array([t(t(t(1.0) * oma) + t(t(k) * a)) for k in (0.5, 0.7, 1.0)], dtype)
            assert_same(got[i], want, f"sky({y!r})")
    mid = ys[np.abs(ys) < 1e30].astype(np.float64)
    assert_same(integrators.sky(mid, "f32"), integrators.sky(mid.astype(np.float32)), "precision=")
    assert_same(got[2], np.array([0.5, t(0.7), 1.0], dtype), "straight up")
    assert_same(got[3], np.ones(3, dtype), "straight down")


@pytest.mark.parametrize("prec", stc.PRECS)
def test_scatter_lanes(prec):
    """The lanes the GPU scatter tests send: ten families, each with lanes that scatter; the camera family's and the
    idle lanes come back as they went; the sized calls interleave misses and invalid rays."""
    assert len(sc.FAMILIES) == 10
    seen = set()
    for fam in sc.FAMILIES:
        la = stc.family_lanes(fam, prec)
        go = la.index >= 0
        assert (go.any() or fam == "camera") and la.index.max() < sc.table().n_spheres and la.sample.max() < 1 << 20
        assert_same(la.want_o[~go], la.o[~go], "o of a miss")
        assert_same(la.want_d[~go], la.d[~go], "d of a miss")
        assert_same(la.want_c[~go], la.c[~go], "colour of a miss")
        if go.any():
            assert (la.want_d[go] != la.d[go]).any(1).mean() > 0.5   # glass met head-on keeps its direction
            seen |= set(np.unique(la.k[go]).tolist())
    assert 0 in seen and 3838 in seen
    assert not stc.family_lanes("mixed", prec).index.min() >= 0
    for n in stc.SIZES:
        la = stc.sized_lanes(prec, n)
        assert la.n == n and (la.k == stc.SIZE_BOUNCE).all()
        if n >= 63:
            assert (la.index == -1).sum() >= 8 and (la.index == -2).sum() >= 8 and (la.index >= 0).sum() > n // 2
            assert np.isnan(la.t[la.index == -2]).all()
