"""GPU parity on degenerate scenes (tests/edge_scenes.py): ties, signed and zero radii, material extremes, the
ends of the numeric range, degenerate lanes and the layout's untested shapes.

Bar: test_gpu_parity.assert_parity's.  The linear image array_equal, the RGB8 bytes equal, ray_segments and the
return code equal to the CPU oracle's: 0 ulp.  tests/test_edge_scenes.py shows on the oracle alone that each
scene reaches the branch it is here for, and pins the oracle on the new behaviour against the independent
restatement.  Every case is at most 48x27 at 32 spp (256 spp on 8x5 for the sample-parallel cases).
"""
import numpy as np
import pytest

import edge_scenes as es
import rt_mi355x as rt
from rt_mi355x import abi
from oracle_bind import oracle_render

pytestmark = pytest.mark.gpu

SEED = es.SEED
F32 = abi.RT_FLAG_F32
SCALAR = abi.RT_FLAG_MODE_SCALAR
PRECS = [0, F32]
PATHS = [0, abi.RT_FLAG_ROOT2, abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_VECTORIZED3, SCALAR]


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    monkeypatch.delenv("RT_FILTER_OFF", raising=False)
    monkeypatch.delenv("RT_WAVES", raising=False)


def gpu(renderer, flat, cam, depth, spp, flags, S=None):
    renderer.seed, renderer.flags = SEED, flags
    return renderer.render_flat(depth, spp, flat, cam, want_linear=True, samples_per_item=S)


_refs = {}


def reference(key, flat, cam, depth, spp, flags):
    """oracle_render, once per key, read-only: shared by the cases that render the same thing twice."""
    if key not in _refs:
        r = oracle_render(flat, cam, depth, spp, SEED, flags & ~F32, precision="f32" if flags & F32 else "f64")
        for a in r[:2]:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def assert_parity(renderer, key, scene, flags, spp=8, depth=50, S=None):
    flat, cam = scene
    rgb_g, lin_g, st, rc_g = gpu(renderer, flat, cam, depth, spp, flags, S)
    rgb_o, lin_o, segs_o, rc_o = reference((key, flags, spp, depth), flat, cam, depth, spp, flags)
    assert rc_g == rc_o
    diff = np.argwhere(lin_g != lin_o)
    assert diff.size == 0, (
        f"{len(diff)} mismatching channels of {lin_o.size}; first pixel {diff[0][0]}: gpu {lin_g[diff[0][0]]} "
        f"oracle {lin_o[diff[0][0]]}")
    np.testing.assert_array_equal(rgb_g, rgb_o)
    assert st.ray_segments == segs_o
    assert st.samples == cam.image_width * cam.image_height * spp
    return lin_g, st


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", PRECS)
def test_twins(renderer, prec, path):
    """Every sphere twice, the copies 1 .. 199 indices apart.  hit_update's three tie rules on the device
    (rt_sweep.hpp:173-212): fp64 select, later scene index wins (:208); the fp32 64-bit key
    (bits(t) - bits(0.001f)) << 32 | ~index (:164-166, :191, :204); scalar mode, earlier index wins (:182).  The
    sweep visits slots, not scene order (rt_layout.hpp, the comment above build_layout): the two grounds and the 2 x 3 big spheres tie
    inside the always-exact group (build_layout's kBigExact rule, rt_sweep.hpp:562-566), the small ones inside clusters that
    hold both members (their centres are equal, so the k-d splits between them rest on the index tie-break,
    build_layout's nth_element comparator), and primary rays tie in camera_exact (rt_camera.hpp:161-162)."""
    assert_parity(renderer, "twins", es.twins(100, 24, 14), prec | path, spp=12)


@pytest.mark.parametrize("path", [0, SCALAR])
@pytest.mark.parametrize("prec", PRECS)
def test_twins_mega(renderer, prec, path):
    """2 200 spheres in pairs through the mega kernels: the ties are found in cluster-local frames (the filter
    sees c' = RN_f(c - C_k), pack_local in rt_layout.hpp, rt_sweep.hpp:591-619; the exact test and hit_update see the
    scene-frame values, so equal t stays equal) under group-local boxes (rt_sweep.hpp:438-457).  Scalar mode
    takes the non-mega kernel over the same layout (pick_kernel in rt_kernel.hip)."""
    _, st = assert_parity(renderer, "twins_mega", es.twins_mega(), prec | path, spp=16)
    if path == 0:
        assert abi.kernel_info(st.kernel_id)["mega"]


@pytest.mark.parametrize("prec", PRECS)
def test_twins_filter_off_same_image(renderer, prec, monkeypatch):
    """test_filter_off_same_image's bar on the twins: with RT_FILTER_OFF=1 every group takes the exact test, so a
    false cull of one member of a tie shows between two GPU renders as well as against the oracle."""
    lin_f, _ = assert_parity(renderer, "twins", es.twins(100, 24, 14), prec, spp=12)
    monkeypatch.setenv("RT_FILTER_OFF", "1")
    lin_x, _ = assert_parity(renderer, "twins", es.twins(100, 24, 14), prec, spp=12)
    np.testing.assert_array_equal(lin_f, lin_x)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", PRECS)
def test_stack(renderer, prec, path):
    """40 coincident spheres: more than one 16-sphere cluster holds, so one tie spans clusters.  Read from
    build_layout (rt_layout.hpp): the ground is always exact (n_xs = 1, n_xg = 1); the 40 are not big
    (equal radii); the k-d node has zero extent on every axis (:191-198, ax stays 0), nth_element orders by scene
    index alone (:202-205) and splits 40 -> 32 | 8 -> 16 | 16 | 8: clusters {1..16}, {17..32}, {33..40} and one
    empty cluster (n_top = 1).  Their three boxes are the same box (pack_sweep, :283-308: centre (0, 1, 0), h =
    1 widened), so a ray passes all or none, walks up to 10 filter groups of identical records, and the tie rule
    alone picks sphere 40 (packed paths) or 1 (scalar).  The best-hit bound never culls a box whose near time
    equals the best t (tn <= bt passes, rt_sweep.hpp:83)."""
    assert_parity(renderer, "stack", es.stack(24, 14), prec | path)


# ---------------------------------------------------------------- signed and zero radii
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", PRECS)
def test_radii(renderer, prec, path):
    """Radii -1, -0.9 (a bubble), -0.2, 0 and 1e-12, and a -r / +r pair.  pack_scene keeps the signed radius for
    scalar mode's normal (p - c) / r (pack_scene in rt_layout.hpp, objects.rs:242) and squares it for everything else (its field()).
    pack_filter floors r2f at floor2 = max(r2max 2^-10, cmax^2 2^-16) (rt_layout.hpp), so the r = 0 and
    r = 1e-12 spheres are filtered as spheres of the floor radius and r2min = floor2, which scales every lane's
    basis (rt_sweep.hpp:396) and every box's kappa (rt_sweep.hpp:414).  The camera cull takes |r| (rt_kernel.hip
    :315, :327) and r^2 (rt_camera.hpp:536)."""
    assert_parity(renderer, "radii", es.radii(24, 14), prec | path)


@pytest.mark.parametrize("name", ["twins", "radii"])
@pytest.mark.parametrize("prec", PRECS)
def test_sample_parallel(renderer, name, prec):
    """The live path again through rt_render_split_async (samples_per_item = 128, 256 spp, 8x5): the oracle's
    image, bytes, segments and rc, and the unsplit render's image, ray_segments and bounce_iters
    (test_gpu_split.check's comparisons).  Ties in trace_paths_split's records; signed radii never reach them."""
    flat, cam = es.twins(100, 8, 5) if name == "twins" else es.radii(8, 5)
    lin_s, st_s = assert_parity(renderer, name + "_split", (flat, cam), prec, spp=256, S=128)
    rgb_u, lin_u, st_u, rc_u = gpu(renderer, flat, cam, 50, 256, prec)
    assert rc_u == 0
    np.testing.assert_array_equal(lin_s, lin_u)
    assert (st_s.ray_segments, st_s.bounce_iters, st_s.samples, st_s.pixels) == \
           (st_u.ray_segments, st_u.bounce_iters, st_u.samples, st_u.pixels)
    assert abi.RT_KERNEL_SPLIT(st_s.kernel_id) and not abi.RT_KERNEL_SPLIT(st_u.kernel_id)


# ---------------------------------------------------------------- material extremes
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("prec", PRECS)
def test_materials(renderer, prec, path):
    """next_ray's scatter branches (rt_camera.hpp:367-458) on the host's MatT precompute (the end of pack_scene, rt_layout.hpp):
    hollow dielectrics, ior 1.5 and 2.4 (the normal negated before the refraction, rt_camera.hpp:442); fuzz
    exactly 1 and fuzz -0.5 (Metal clamps only above); albedo 1 metal; ior 1 (qf = qb = 0), 0.7, 1e-3 and 1e3
    (inv = 1/ior, qf, qb rounded once on the host in T, :41-45); Lambertian albedo 0 and 1."""
    assert_parity(renderer, "materials", es.materials(24, 14), prec | path)


# ---------------------------------------------------------------- numeric range
@pytest.mark.parametrize("s", es.SCALES)
@pytest.mark.parametrize("prec", PRECS)
def test_scaled(renderer, prec, s):
    """random_spheres(100) and its camera scaled by s.  The fp32 culls sit in front of the exact test in T, so an
    fp64 render must survive them at every scale.  Read from the code:
      1e6, 1e12: ordinary lanes, pm = f_cmax + |o|_1 <= 1e15 (rt_sweep.hpp:417), margin ~ 48 u pm^2.
      1e14 and above: f_cmax alone is over 1e15, every lane of the general sweep takes the zero basis and zero
        box times (rt_sweep.hpp:417-421): every box and every sphere passes to the exact test.
      1e19, fp32 render: the ground's r^2 = 1e44 is +inf in T (always exact: pack_filter's `finite` rule), the other r2f
        are finite (big 1e38, small 4e36 = r2min, f_ir2 = 2.5e-37); |c|^2 overflows in the exact test, every
        discriminant is -inf or NaN; build_cam_table's c = +inf gives sc = +inf (rt_camera.hpp:494-498): sky.
      1e19 and 1e25, fp64 render: the fp32 squares of the cone cull's |w x a| (rt_camera.hpp:69-71) overflow for
        |w| over 1.8e19, f = +inf > rp culled every sphere and the primary rays saw only sky (the first run of
        these cases: 594 of 1008 channels wrong); build_cam_table now gives records with |w| >= 1e18 rp = +inf,
        always tested (kConeWMax, rt_camera.hpp:503-509, :535, :552), next to rup's 1e30 rule (:510-511).
      1e25, fp32 render: every r^2 is +inf in T, so pack_filter's isfinite rules (both of its loops) make every
        r2f +inf and leave cmax = r2max = 0, while build_layout's rule on the fp64 scene (:148) still puts all but
        the ground into clusters; no sphere is filtered: r2min = 0 (the end of pack_filter), f_ir2 = f_hir2 = f_isr = +inf (build_tables), f_cmax = 0, the cluster
        boxes have h = +inf and a NaN centre (pack_sweep's cluster boxes), which passes (rt_sweep.hpp:102, NaN: kept).
      1e25, fp64 render: r2f = round_up_f32(4e48) = +inf through pack_filter's finite branch, so r2max = +inf,
        r2min = 0 as above; the general sweep's lanes are all degenerate, the exact test in double has the range.
    At 1e19 and 1e25 the fp32 oracle renders pure sky with one segment per sample (test_edge_scenes.py); at the
    other scales 59.5 % of the pixels see the scene, in fp64 at every scale."""
    assert_parity(renderer, ("scaled", s), es.scaled(s), prec)


@pytest.mark.parametrize("s", [1e16, 1e25])
def test_scaled_scalar_f64(renderer, s):
    """Scalar mode (no FMA, both roots, the signed-radius normal) at the scales where every lane is degenerate."""
    assert_parity(renderer, ("scaled", s), es.scaled(s), SCALAR)


# ---------------------------------------------------------------- degenerate lanes
@pytest.mark.parametrize("path", [0, SCALAR])
@pytest.mark.parametrize("kind", es.NEEDLES)
@pytest.mark.parametrize("prec", PRECS)
def test_needle(renderer, prec, kind, path):
    """Rays all but parallel to an axis, primary rays included (the -0.0 in the camera centre, or the defocus
    disk, keeps the launch off the camera batches: frame_params' pinhole test in rt_kernel.hip).  down_1e-6: L = fx^2 + fz^2 straddles
    1e-15 (rt_sweep.hpp:417), 22 % of the primary rays below it, so waves mix lanes with a zero basis and zero
    box times with ordinary lanes whose basis is scaled by rsq(L) up to 3e7 (rt_sweep.hpp:397).  down_1e-30 and
    down_defocus: every primary lane degenerate, the bounced rays ordinary.  along_x: d = (1, 0, 0) exactly or
    within 1e-20, so inv_ax clamps the y and z components to +-1e-20 keeping the sign, -0.0 included
    (rt_sweep.hpp:410-413): slab times of 1e20 times the offset."""
    assert_parity(renderer, ("needle", kind), es.needle(kind), prec | path)


@pytest.mark.parametrize("prec", PRECS)
def test_needle_filter_off_same_image(renderer, prec, monkeypatch):
    """down_1e-6 with and without the filter: the same image (test_filter_off_same_image's bar)."""
    lin_f, _ = assert_parity(renderer, ("needle", "down_1e-6"), es.needle("down_1e-6"), prec)
    monkeypatch.setenv("RT_FILTER_OFF", "1")
    lin_x, _ = assert_parity(renderer, ("needle", "down_1e-6"), es.needle("down_1e-6"), prec)
    np.testing.assert_array_equal(lin_f, lin_x)


# ---------------------------------------------------------------- layout statistics
@pytest.mark.parametrize("name", sorted(es.LAYOUT_FAMILIES))
@pytest.mark.parametrize("prec", PRECS)
def test_layout_families(renderer, prec, name):
    """build_layout's untested shapes (rt_layout.hpp).
      concentric, collinear, coplanar: k-d nodes with zero extent on 3, 2 and 1 axes (:191-198); the split then
        rests on the comparator's index tie-break (:202-205), in build and in kd_order (:216-235).
      big8: 8 = kBigExact big spheres join the always-exact group and are alone in it (:164-168; n_xs = 8, two
        whole groups, no dummy pair to skip at rt_sweep.hpp:563).  big9: one more and all stay in the clusters.
      uniform, big9, concentric, count1: no always-exact sphere at all: n_xs = n_xg = 0, the exact loop
        (rt_sweep.hpp:562) and cone_walk's first level (rt_camera.hpp:79) run zero times, xw0 is the pad record.
      count n: 1, 2, 5, 15, 16 (one full cluster), 17 (16 + 1 after the N <= kClusterMax leaf of its build()), 33, 64 (one
        super), 65 (unit 64: 64 | 1 with the left child's clusters padded to 4, :199-208).
      count1, read: median = the sphere's own key, nothing exact, nothing big (r > 3 r is false), one cluster of
        one member padded to 4 clusters (:212), n_top = 1, slots 0 .. 15 with 15 dummies (r2f = -inf never pass,
        r^2 = -inf never hit), the super box equals the cluster box, n_mg = 0; launch_plain picks the small-launch
        kernel (fp32 W5, fp64 W4) with camera batches, and the pixel lists hold at most slot 0."""
    flat, cam = es.LAYOUT_FAMILIES[name]()
    assert_parity(renderer, ("layout", name), (flat, cam), prec)
