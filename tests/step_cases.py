"""Path steps (rt_scatter_async, rt_path_step_async): the inputs and expectations tests/test_step_cases.py (CPU: the
expectations proven with the oracle alone) and the GPU tests (tests/test_gpu_scatter_api.py, tests/test_gpu_path_step.py)
share.

Plain module: no GPU, no fixtures, deterministic.  Two things:
  * the loop that must equal a render: a camera's own primary rays (oracle_get_ray; pixel = row W + col, sample = s,
    pixel-major), and Scene::trace_vectorized written as a loop of steps over oracle_nearest_hit + oracle_next_ray +
    rt_mi355x.integrators.sky, which tests/test_step_cases.py holds against oracle_render(flags = MODE_VECTORIZED);
  * the lanes of tests/scatter_cases.py (imported, not edited) laid out as rt_scatter_async takes them, with miss and
    invalid lanes interleaved, and their reference, oracle_next_ray.
Every reference is computed once per key and left unchanged (read-only arrays).
"""
import functools

import numpy as np

import oracle_bind as ob
import query_cases as qc
import rt_mi355x as rt
import scatter_cases as sc
from rt_mi355x import abi, integrators

SEED = 0x5EED0001
W, H = 16, 9
BOUNCES = 8
SPPS = (1, 4, 6)           # 6: a partial chunk
LONG = (50, 4)             # once: 50 bounces at 4 spp
PRECS = ("f64", "f32")
MODES = ("packed", "root2")
DTYPES = {"f32": np.float32, "f64": np.float64}
V1 = abi.RT_FLAG_MODE_VECTORIZED


@functools.lru_cache(maxsize=None)
def scene():
    return rt.scenes.random_spheres(100).flatten()


@functools.lru_cache(maxsize=None)
def camera():
    return rt.camera_new_py(W, H, **rt.MAIN_CAMERA)


def render_flags(prec, mode):
    """The flags of the render the loop must equal (oracle_render takes the precision apart from them)."""
    return V1 | (abi.RT_FLAG_ROOT2 if mode == "root2" else 0)


@functools.lru_cache(maxsize=None)
def primary_rays(prec, spp):
    """The camera's own primary rays, pixel-major with a pixel's samples in order: (o [n, 3], d [n, 3], pixel [n],
    sample [n]), n = W H spp."""
    pix = np.repeat(np.arange(W * H, dtype=np.uint32), spp)
    sid = np.tile(np.arange(spp, dtype=np.uint32), W * H)
    o, d = ob.oracle_get_ray(DTYPES[prec], camera(), SEED, pix % W, pix // W, pix, sid)
    out = (np.ascontiguousarray(o.T), np.ascontiguousarray(d.T), pix, sid)
    for a in out:
        a.setflags(write=False)
    return out


class LoopResult:
    """radiance [n, 3] per ray, invalid (lanes that violated the query's precondition while alive, summed over the
    steps), segments (the alive rays summed over the steps: a render's ray_segments), and per step k the arrays after
    it: status [n] (abi.RT_STEP_*; retired rays 255), o, d, colour, and the normal of the step's hits."""


def cpu_loop(prec, mode, spp, bounces, keep_steps=False):
    """Scene::trace_vectorized as a loop of steps with the oracle's probes: the colour starts at 1; for k in
    0..bounces a hit scatters (oracle_next_ray), a miss multiplies by sky(d.y) of its own final direction and retires;
    a ray still alive at the end is 0."""
    flat = scene()
    o, d, pix, sid = (a.copy() for a in primary_rays(prec, spp))
    n = d.shape[0]
    dtype = d.dtype
    colour = np.ones((n, 3), dtype)
    alive = np.ones(n, bool)
    missed = np.zeros(n, bool)
    res = LoopResult()
    res.invalid, res.segments, res.steps = 0, 0, []
    for k in range(bounces):
        if not alive.any():
            break
        a = np.flatnonzero(alive)
        ok = qc.valid_fast(o[a], d[a])
        res.invalid += int((~ok).sum())
        res.segments += a.size
        idx, t = ob.oracle_nearest_hit(flat, mode, np.ascontiguousarray(o[a].T), np.ascontiguousarray(d[a].T))
        hit = a[idx >= 0]
        status = np.full(n, abi.RT_STEP_INVALID, np.uint8)
        status[a] = abi.RT_STEP_MISSED
        normal = np.zeros((n, 3), dtype)
        if hit.size:
            status[hit] = abi.RT_STEP_SCATTERED
            oo, dd, cc, nn, _, _ = ob.oracle_next_ray(flat, SEED, "packed", np.ascontiguousarray(o[hit].T),
                                                    np.ascontiguousarray(d[hit].T), idx[idx >= 0], t[idx >= 0], sid[hit],
                                                    pix[hit], np.full(hit.size, k, np.uint32),
                                                    np.ascontiguousarray(colour[hit].T))
            o[hit], d[hit], colour[hit], normal[hit] = oo.T, dd.T, cc.T, nn.T
        gone = a[idx < 0]
        missed[gone] = True
        alive[gone] = False
        if keep_steps:
            res.steps.append((status, o.copy(), d.copy(), colour.copy(), normal))
    radiance = np.zeros((n, 3), dtype)
    radiance[missed] = colour[missed] * integrators.sky(d[missed, 1])
    res.radiance = radiance
    return res


@functools.lru_cache(maxsize=None)
def loop(prec, mode, spp, bounces=BOUNCES):
    res = cpu_loop(prec, mode, spp, bounces)
    res.radiance.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def render(prec, mode, spp, bounces=BOUNCES):
    """oracle_render in mode "vectorized": (linear [W H, 3] float64, segments)."""
    _, lin, segs, rc = ob.oracle_render(scene(), camera(), bounces, spp, SEED, flags=render_flags(prec, mode), precision=prec)
    assert rc == 0
    lin.setflags(write=False)
    return lin, segs


# The lights of the direct_light test: one inside the ground sphere (centre (0, -1000, 0), radius 1000), where a hit on
# the ground has the light behind its surface and a hit anywhere else has the ground in the way; one in the open.
LIGHT_INSIDE = (0.0, -500.0, 0.0)
LIGHT_OPEN = (0.0, 30.0, 0.0)


def lit_lanes(prec, light, spp=4):
    """Per step of the CPU loop, the lanes a light reaches by integrators.direct_light's rule, judged with the oracle:
    scattered, the light in front of the hit's normal, and no accepted root of the shadow ray (integrators.shadow_rays)
    below its t_max.  Returns (lit lanes summed over the steps, shadow rays summed over the steps)."""
    res = cpu_loop(prec, "packed", spp, BOUNCES, keep_steps=True)
    lit = rays = 0
    for status, o, _, _, normal in res.steps:
        s = np.flatnonzero(status == abi.RT_STEP_SCATTERED)
        sd, dist = integrators.shadow_rays(o[s], light)
        assert qc.valid_fast(o[s], sd).all()
        idx, t = ob.oracle_nearest_hit(scene(), "packed", np.ascontiguousarray(o[s].T), np.ascontiguousarray(sd.T))
        occluded = (idx >= 0) & (t < dist)
        cos = np.einsum("ij,ij->i", normal[s], sd)
        lit += int((~occluded & (cos > 0)).sum())
        rays += s.size
    return lit, rays


# ---------------------------------------------------------------- scatter lanes in the entry point's layout
SIZES = (1, 63, 64, 65, 300)
SIZE_BOUNCE = 7


class ScatterLanes:
    """Lanes as rt_scatter_async takes them: o, d, c [n, 3], index [n] int32, t [n], pixel, sample, k [n] uint32 (a
    call has one bounce: the lanes with k == bounce are the call's hits), and the expected want_o, want_d, want_c
    [n, 3]: oracle_next_ray for index >= 0, the inputs otherwise."""


def _reference(call):
    go = np.flatnonzero(call.index >= 0)
    call.want_o, call.want_d, call.want_c = call.o.copy(), call.d.copy(), call.c.copy()
    if go.size:
        oo, dd, cc, _, _, _ = ob.oracle_next_ray(sc.table(), sc.SEED, "packed", np.ascontiguousarray(call.o[go].T),
                                                np.ascontiguousarray(call.d[go].T), call.index[go], call.t[go],
                                                call.sample[go], call.pixel[go], call.k[go],
                                                np.ascontiguousarray(call.c[go].T))
        call.want_o[go], call.want_d[go], call.want_c[go] = oo.T, dd.T, cc.T
    call.n = call.index.size
    for a in vars(call).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return call


def _from_lanes(la, dtype):
    call = ScatterLanes()
    call.o, call.d, call.c = (np.ascontiguousarray(getattr(la, f).T) for f in ("o", "d", "c"))
    scatter = la.role == sc.SCATTER
    call.index = np.where(scatter, la.hit_i, -1).astype(np.int32)   # a camera or idle lane of the family: a miss
    call.t = np.where(scatter, la.hit_t, np.inf).astype(dtype)
    call.pixel, call.sample, call.k = la.pix.copy(), la.sid.copy(), la.k.copy()
    return call


@functools.lru_cache(maxsize=None)
def family_lanes(family, prec):
    """Every lane of a family of tests/scatter_cases.py (the packed mode: next_ray<T, false>), in the family's own
    order, so that its waves stay mixed as it built them; camera and idle lanes are misses, to be handed back bit for
    bit.  The scene is scatter_cases.table(), the seed scatter_cases.SEED."""
    la = sc.Lanes.cat([ln.lanes for ln in sc.family(family, prec, "packed")])
    return _reference(_from_lanes(la, DTYPES[prec]))


@functools.lru_cache(maxsize=None)
def sized_lanes(prec, n):
    """The first n ordinary lanes with one bounce for all of them (the ordinary family aims at no draw of its own);
    lanes 3, 10, 17, .. are misses (-1, t +inf) and lanes 5, 12, 19, .. invalid rays (-2, t NaN), their o, d and
    colour kept: to be handed back bit for bit."""
    la = sc.ordinary_lanes(prec, "packed").take(np.arange(n))
    call = _from_lanes(la, DTYPES[prec])
    call.k[:] = SIZE_BOUNCE
    call.index[3::7], call.t[3::7] = abi.RT_QUERY_MISS, np.inf
    call.index[5::7], call.t[5::7] = abi.RT_QUERY_INVALID, np.nan
    return _reference(call)
