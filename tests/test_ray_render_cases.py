"""The inputs of tests/test_gpu_ray_render.py and the host ray generators (rt_camera_rays), without a GPU.

* The two references of tests/ray_render_cases.py agree bit for bit on the R = 1 ray sets in both precisions, so the
  GPU test's expected values do not rest on one restatement; the sets hold what their docstrings promise (rays that
  start inside a sphere, rays that miss everything, directions at both bounds of the precondition).
* rt_camera_rays: every ray inside the image satisfies the precondition (query_cases.valid_rays), orthographic
  directions are bitwise equal and the origins all differ, panorama and fisheye origins all equal (T)center, the ray
  through an odd-sized image's centre pixel at grid = 1 is the double-rounded view axis, and the fisheye pixels with
  r > 1 are exactly the zero directions.
"""
import ctypes

import numpy as np
import pytest

import query_cases as qc
import ray_render_cases as rc
import rt_mi355x as rt
from oracle_bind import oracle_nearest_hit
from rt_mi355x import abi

FROM, AT, UP = (13.0, 2.0, 3.0), (0.5, 0.25, -0.125), (0.0, 1.0, 0.0)


def view_axis():
    v = np.array(AT) - np.array(FROM)
    return v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("prec", rc.PRECS)
def test_references_agree_on_single_rays(prec):
    flat = rc.scene("s100")
    o, tgt, d = rc.ray_set(prec)
    sel = np.r_[0:14, 60:66]   # inside, sky and field rays (reference B is Python: a subset keeps this quick)
    for spp, depth in ((6, 8), (1, 1), (5, 3)):
        rgb_a, lin_a, segs_a, rc_a = rc.reference_a(flat, o[sel], tgt[sel], spp, depth, prec, pixel_base=77)
        rgb_b, lin_b, segs_b, rc_b = rc.reference_b(flat, o[sel, None, :], d[sel, None, :], spp, depth, prec, pixel_base=77)
        assert rc_a == rc_b
        qc.assert_same(lin_b, lin_a, f"{prec} spp {spp} depth {depth}")
        assert np.array_equal(rgb_a, rgb_b) and segs_a == segs_b


@pytest.mark.parametrize("prec", rc.PRECS)
def test_ray_sets_hold_what_they_promise(prec):
    flat = rc.scene("s100")
    o, tgt, d = rc.ray_set(prec)
    assert o.shape == d.shape == (rc.N_PIX, 3) and o.dtype == d.dtype == rc.DTYPES[prec]
    assert qc.valid_rays(o, d).all()
    cen, rad = flat.center, flat.radius
    inside = (np.linalg.norm(o[:, None, :].astype(np.float64) - cen[None], axis=-1) < np.abs(rad)[None]).any(1)
    assert inside[:rc.N_INSIDE].all() and not inside[rc.N_INSIDE:].any()
    idx, _ = oracle_nearest_hit(flat, "root2", np.ascontiguousarray(o.T), np.ascontiguousarray(d.T))
    assert (idx[rc.N_INSIDE:rc.N_INSIDE + rc.N_SKY] == -1).all(), "the sky rays miss every sphere"
    assert (idx[:rc.N_INSIDE] >= 0).all() and (idx >= 0).sum() > 100
    # the per-sample sets: every ray valid, and the two bound rays one step inside the precondition's edge
    T = rc.DTYPES[prec]
    lo, hi = rc.bound_lengths(T)
    for R in (2, 3, 7):
        po, pd = rc.per_sample_rays(prec, R)
        assert po.shape == pd.shape == (12, R, 3) and qc.valid_rays(po.reshape(-1, 3), pd.reshape(-1, 3)).all()
        assert pd[0, 0, 0] == lo and pd[1, 0, 2] == -hi
    edge = np.array([[np.nextafter(lo, T(0)), 0, 0], [lo, 0, 0], [0, hi, 0], [0, np.nextafter(hi, T(np.inf)), 0]], T)
    assert qc.valid_rays(np.zeros(3), edge).tolist() == [False, True, True, False]
    l2 = (pd.astype(np.float64) ** 2).sum(-1)
    assert l2.min() < 1e-4 and l2.max() > 1e4, "the lengths spread over the admitted range"


# ---------------------------------------------------------------- rt_camera_rays
@pytest.mark.parametrize("prec", rc.PRECS)
@pytest.mark.parametrize("grid", (1, 3))
def test_orthographic(prec, grid):
    W, H = 9, 5
    o, d = rt.projections.orthographic(W, H, FROM, AT, UP, extent=6.0, grid=grid, precision=prec)
    T = rc.DTYPES[prec]
    assert o.shape == d.shape == (W * H, grid * grid, 3) and o.dtype == d.dtype == T
    flat_o, flat_d = o.reshape(-1, 3), d.reshape(-1, 3)
    assert qc.valid_rays(flat_o, flat_d).all()
    assert (qc.bits(flat_d) == qc.bits(flat_d[0])[None]).all(), "one direction, bit for bit"
    assert np.array_equal(flat_d[0], view_axis().astype(T))
    assert len({r.tobytes() for r in flat_o}) == flat_o.shape[0], "every origin differs"
    # the plane through the centre, `extent` high and extent * W / H wide, the centre ray from the centre itself
    if grid == 1:
        assert np.array_equal(o[(H // 2) * W + W // 2, 0], np.array(FROM).astype(T))
    span = flat_o.astype(np.float64) - np.array(FROM)
    assert np.abs(span @ view_axis()).max() < 1e-5
    assert abs(np.linalg.norm(span, axis=1).max() - 0.5 * np.hypot(6.0 * W / H, 6.0) * (1 - 1 / (max(W, H) * grid))) < 0.7


@pytest.mark.parametrize("prec", rc.PRECS)
@pytest.mark.parametrize("model", ("equirect", "fisheye"))
def test_panorama_and_fisheye(model, prec):
    W, H, T = 11, 7, rc.DTYPES[prec]
    for grid in (1, 2):
        o, d = rt.projections.camera_rays(model, W, H, FROM, AT, UP, grid=grid, precision=prec, angle_deg=200.0)
        assert o.shape == d.shape == (W * H, grid * grid, 3) and o.dtype == d.dtype == T
        assert (o == np.array(FROM).astype(T)[None, None, :]).all(), "one origin: (T)center"
        fo, fd = o.reshape(-1, 3), d.reshape(-1, 3)
        zero = (fd == 0).all(1)
        if model == "equirect":
            assert not zero.any()
        else:   # r restated in double: the distance from the image centre in units of half the shorter side
            j, i = np.divmod(np.arange(grid * grid), grid)
            row, col = np.divmod(np.arange(W * H), W)
            x = (col[:, None] + (i[None, :] + 0.5) / grid) - W / 2.0
            y = (row[:, None] + (j[None, :] + 0.5) / grid) - H / 2.0
            r = np.sqrt(x * x + y * y) / (H / 2.0)
            assert np.array_equal(zero.reshape(W * H, -1), r > 1.0) and zero.any() and not zero.all()
        assert qc.valid_rays(fo[~zero], fd[~zero]).all() and not qc.valid_rays(fo[zero], fd[zero]).any()
        n2 = (fd[~zero].astype(np.float64) ** 2).sum(1)
        assert np.abs(n2 - 1).max() < (1e-6 if prec == "f32" else 1e-14), "unit in double, rounded last"
        if grid == 1:
            assert np.array_equal(d[(H // 2) * W + W // 2, 0], view_axis().astype(T)), "the centre pixel: the view axis"
    # the layout: a panorama's columns turn about `up`, its top row looks up; a fisheye's rim is angle / 2 off the axis
    o, d = rt.projections.camera_rays(model, W, H, FROM, AT, UP, grid=1, precision="f64", angle_deg=200.0)
    d = d.reshape(H, W, 3)
    ax = view_axis()
    if model == "equirect":
        assert d[0, :, 1].min() > 0.8 and d[-1, :, 1].max() < -0.8
        assert d[H // 2, 0] @ ax < -0.9 and d[H // 2, W // 2] @ ax > 0.999
        right = np.cross(ax, UP)
        assert d[H // 2, 3 * W // 4] @ right > 0.5 and d[H // 2, W // 4] @ right < -0.5
    else:
        top = d[0, W // 2]   # r = (H/2 - 0.5) / (H/2), straight up in the image
        ang = np.degrees(np.arccos(top @ ax))
        assert abs(ang - (1 - 1 / H) * 100.0) < 1e-9 and top[1] > d[H // 2, W // 2][1]


def test_camera_rays_refusals(lib):
    buf = (ctypes.c_double * (3 * 64))()

    def call(model=0, w=4, h=4, grid=1, flags=0, at=AT, up=UP, angle=180.0, extent=1.0, o=buf, d=buf, null=False):
        p = abi.RtProjection(model, w, h, (abi.f64 * 3)(*FROM), (abi.f64 * 3)(*at), (abi.f64 * 3)(*up), angle, extent)
        return lib.rt_camera_rays(None if null else ctypes.byref(p), grid, flags, o, d)

    assert call() == abi.RT_OK
    for what, kw in (("NULL projection", dict(null=True)), ("NULL origins", dict(o=None)), ("NULL directions", dict(d=None)),
                     ("empty image", dict(w=0)), ("empty image", dict(h=0)), ("grid 0", dict(grid=0)),
                     ("unknown model", dict(model=3)), ("unknown flag", dict(flags=abi.RT_FLAG_ROOT2)),
                     ("look_at == center", dict(at=FROM)), ("up along the axis", dict(up=tuple(view_axis()))),
                     ("non-finite", dict(at=(np.nan, 0, 0))), ("fisheye angle", dict(model=2, angle=0.0)),
                     ("fisheye angle", dict(model=2, angle=361.0)), ("ortho extent", dict(extent=0.0)),
                     ("ortho extent", dict(extent=np.inf))):
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert b"rt_camera_rays" in lib.rt_last_error()
    assert call(w=0x10000, h=0x8000, o=None) == abi.RT_ERR_INVALID   # the NULL check comes first
    assert call(w=0x10000, h=0x8000) == abi.RT_ERR_UNSUPPORTED and call(grid=1025) == abi.RT_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="unknown projection"):
        rt.projections.camera_rays("pinhole", 4, 4, FROM, AT)
    with pytest.raises(ValueError, match="precision"):
        rt.projections.equirect(4, 4, FROM, AT, precision="f16")
    with pytest.raises(ValueError, match="positive"):
        rt.projections.equirect(4, 0, FROM, AT)
