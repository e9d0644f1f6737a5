"""Integrators driven from the host over the path steps (GpuRenderer.path_step_into, occluded_into): what a caller
builds once the material stage is public.  path_trace is the reference's Scene::trace_vectorized as a loop of steps
(bit for bit a render in mode "vectorized" for a camera's own primary rays); direct_light adds what the reference
cannot do, a point light with one shadow ray per hit.  Both keep the rays on the device between steps and move one
status byte and the directions of each step to the host, where the caller's own rules (the sky, retiring, the light)
run in numpy.  path_trace(compact=True) instead steps over ray lists compacted on the device and moves 4 bytes per step.
"""
import numpy as np

from . import abi
from .renderer import _flat


def sky(dy, precision=None):
    """The device's sky() in numpy, the same operations in the same order (ray_tracing.rs:490-494): a = (y + 1) 0.5,
    then per channel 1 (1 - a) + k a with k = 0.5, 0.7, 1.  dy: (n,) y components of the final directions; precision:
    "f32" or "f64" (None: dy's dtype).  Returns (n, 3) in that precision."""
    T = np.dtype({"f32": np.float32, "f64": np.float64}[precision] if precision else np.asarray(dy).dtype).type
    with np.errstate(all="ignore"):
        y = np.asarray(dy, dtype=T)
        a = (y + T(1.0)) * T(0.5)
        oma = -a + T(1.0)
        return np.stack([T(1.0) * oma + T(k) * a for k in (0.5, 0.7, 1.0)], axis=-1)


class DeviceArray:
    """A device allocation of a DeviceScope with a shape and a dtype, exposing __cuda_array_interface__: what the
    renderer's _into methods take when the caller has no tensor library."""

    def __init__(self, dev, a=None, shape=None, dtype=None):
        self.dev = dev
        self.shape, self.dtype = (a.shape, a.dtype) if a is not None else (tuple(shape), np.dtype(dtype))
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = dev.upload(np.ascontiguousarray(a)) if a is not None else dev.alloc(max(self.nbytes, 1))

    @property
    def __cuda_array_interface__(self):
        return {"shape": tuple(self.shape), "typestr": self.dtype.str, "data": (self.ptr.value, False), "version": 3}

    def get(self):
        return self.dev.download(self.ptr, np.empty(self.shape, dtype=self.dtype))

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        abi.check(self.dev.lib, self.dev.lib.rt_memcpy_h2d(self.dev.ctx, self.ptr, a.ctypes.data, a.nbytes))


def shadow_rays(points, light, mask=None):
    """The shadow rays of direct_light: from each point (n, 3) towards the light, unit directions (so a root counts
    from 0.001 world units on, as in a render) with t_max the distance: (directions (n, 3), t_max (n,)) in the points'
    precision.  Rows outside `mask` get a zero direction: an invalid ray, not traced."""
    p = np.asarray(points)
    v = np.asarray(light, dtype=p.dtype) - p
    dist = np.sqrt(np.einsum("ij,ij->i", v, v))
    ok = dist > 0 if mask is None else (mask & (dist > 0))
    sd = np.zeros_like(p)
    sd[ok] = v[ok] / dist[ok, None]
    return sd, np.where(ok, dist, 0).astype(p.dtype)


def _loop(renderer, origins, directions, pixel, sample, max_bounces, scene, seed, root2, stats, light):
    T = np.dtype(np.float32 if renderer.flags & abi.RT_FLAG_F32 else np.float64)
    o = np.array(origins, dtype=T, order="C")
    d = np.array(directions, dtype=T, order="C")
    n = d.shape[0]
    pixel = np.arange(n, dtype=np.uint32) if pixel is None else np.ascontiguousarray(pixel, dtype=np.uint32)
    sample = np.zeros(n, dtype=np.uint32) if sample is None else np.ascontiguousarray(sample, dtype=np.uint32)
    radiance = np.zeros((n, 3), dtype=T)
    totals = {"ray_segments": 0, "samples": 0, "kernel_ms": 0.0, "steps": 0, "invalid": 0, "shadow_rays": 0}
    if stats is not None:
        stats.update(totals)
    if n == 0:
        return radiance
    renderer._use_scene(_flat(scene))
    alive = np.ones(n, dtype=bool)     # still carrying a path
    final_dy = np.zeros(n, dtype=T)    # the y of a missed ray's own final direction
    missed = np.zeros(n, dtype=bool)
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        d_o, d_d = DeviceArray(dev, o), DeviceArray(dev, d)
        d_c = DeviceArray(dev, np.ones((n, 3), dtype=T))
        d_pix, d_smp = DeviceArray(dev, pixel), DeviceArray(dev, sample)
        d_st = DeviceArray(dev, shape=(n,), dtype=np.uint8)
        d_nrm = d_sd = d_tm = d_occ = None
        if light is not None:
            d_nrm = DeviceArray(dev, shape=(n, 3), dtype=T)
            d_sd = DeviceArray(dev, shape=(n, 3), dtype=T)
            d_tm = DeviceArray(dev, shape=(n,), dtype=T)
            d_occ = DeviceArray(dev, shape=(n,), dtype=np.uint8)
        for k in range(max_bounces):
            if not alive.any():
                break
            renderer.path_step_into(d_o, d_d, d_pix, d_smp, bounce=k, colour=d_c, status=d_st, normal=d_nrm, seed=seed,
                                    root2=root2)
            st, _ = abi.collect(renderer.lib, renderer.ctx)
            totals["ray_segments"] += st.ray_segments
            totals["samples"] += st.samples
            totals["kernel_ms"] += st.kernel_ms
            totals["steps"] += 1
            status = d_st.get()
            totals["invalid"] += int(np.count_nonzero(alive & (status == abi.RT_STEP_INVALID)))
            now_missed = alive & (status != abi.RT_STEP_SCATTERED)
            scattered = alive & (status == abi.RT_STEP_SCATTERED)
            if light is not None and scattered.any():
                # next-event estimation: one shadow ray per hit, from the hit point (the new origin) towards the light
                pos, intensity = light
                p, nrm, col = d_o.get(), d_nrm.get(), d_c.get()
                sd, dist = shadow_rays(p, pos, scattered)
                d_sd.set(sd)
                d_tm.set(dist)
                renderer.occluded_into(d_o, d_sd, d_occ, t_max=d_tm, root2=root2)
                sst, _ = abi.collect(renderer.lib, renderer.ctx)
                totals["kernel_ms"] += sst.kernel_ms
                totals["shadow_rays"] += sst.samples
                cos = np.einsum("ij,ij->i", nrm, sd)
                lit = scattered & (d_occ.get() == abi.RT_OCCLUDED_NO) & (cos > 0)
                if lit.any():
                    w = (cos[lit] / (dist[lit] * dist[lit]))[:, None]
                    radiance[lit] += col[lit] * np.asarray(intensity, dtype=T) * w
            if now_missed.any():
                dn = d_d.get()
                final_dy[now_missed] = dn[now_missed, 1]
                missed |= now_missed
                alive &= ~now_missed
                dn[now_missed] = 0   # retired: an invalid ray from here on, not traced
                d_d.set(dn)
        colour = d_c.get()
    # a miss multiplies by the sky of the ray's own final direction; a ray still alive at the end is 0
    radiance[missed] += colour[missed] * sky(final_dy[missed])
    if stats is not None:
        stats.update(totals)
    return radiance


def _loop_lists(renderer, origins, directions, pixel, sample, max_bounces, scene, seed, root2, stats):
    """path_trace over ray lists: each step runs over the rays the last one scattered (rt_path_step_list_async) and
    leaves the next list on the device; the host reads the 4-byte count after each step and the status, the directions
    and the colour once at the end.  A retired ray is simply no longer listed: its final direction, colour and last
    status stay where they are."""
    T = np.dtype(np.float32 if renderer.flags & abi.RT_FLAG_F32 else np.float64)
    o = np.array(origins, dtype=T, order="C")
    d = np.array(directions, dtype=T, order="C")
    n = d.shape[0]
    pixel = np.arange(n, dtype=np.uint32) if pixel is None else np.ascontiguousarray(pixel, dtype=np.uint32)
    sample = np.zeros(n, dtype=np.uint32) if sample is None else np.ascontiguousarray(sample, dtype=np.uint32)
    radiance = np.zeros((n, 3), dtype=T)
    totals = {"ray_segments": 0, "samples": 0, "kernel_ms": 0.0, "steps": 0, "invalid": 0, "shadow_rays": 0}
    if stats is not None:
        stats.update(totals)
    if n == 0:
        return radiance
    renderer._use_scene(_flat(scene))
    with abi.DeviceScope(renderer.lib, renderer.ctx) as dev:
        d_o, d_d = DeviceArray(dev, o), DeviceArray(dev, d)
        d_c = DeviceArray(dev, np.ones((n, 3), dtype=T))
        d_pix, d_smp = DeviceArray(dev, pixel), DeviceArray(dev, sample)
        d_st = DeviceArray(dev, np.zeros(n, dtype=np.uint8))   # a ray that is never stepped (max_bounces 0) is not a miss
        lists = [DeviceArray(dev, shape=(n,), dtype=np.uint32) for _ in range(2)]
        counts = [DeviceArray(dev, shape=(1,), dtype=np.uint32) for _ in range(2)]
        live = n
        for k in range(max_bounces):
            if live == 0:
                break
            src, dst = (k + 1) % 2, k % 2
            renderer.path_step_list_into(d_o, d_d, d_pix, d_smp, bounce=k, list_in=lists[src] if k else None,
                                         count_in=counts[src] if k else None, list_out=lists[dst], count_out=counts[dst],
                                         colour=d_c, status=d_st, seed=seed, root2=root2)
            st, _ = abi.collect(renderer.lib, renderer.ctx)
            totals["ray_segments"] += st.ray_segments
            totals["samples"] += st.samples
            totals["kernel_ms"] += st.kernel_ms
            totals["steps"] += 1
            live = int(counts[dst].get()[0])
        status, dn, colour = d_st.get(), d_d.get(), d_c.get()
    if max_bounces > 0:
        missed = status == abi.RT_STEP_MISSED
        totals["invalid"] = int(np.count_nonzero(status == abi.RT_STEP_INVALID))
        # a miss multiplies by the sky of the ray's own final direction; a ray still alive at the end is 0
        radiance[missed] += colour[missed] * sky(dn[missed, 1])
    if stats is not None:
        stats.update(totals)
    return radiance


def path_trace(renderer, origins, directions, pixel, sample, max_bounces, scene, seed=None, root2=False, stats=None,
               compact=False):
    """Scene::trace_vectorized as a loop over rt_path_step_async: the colour starts at 1; for k in 0..max_bounces a
    hit scatters, a miss multiplies by sky(d.y) of the ray's own final direction and retires (its direction is zeroed,
    so later steps do not trace it); a ray still alive at the end is 0.  origins, directions: (n, 3); pixel, sample:
    (n,) integers keying each ray's draws (None: arange(n) and zeros); seed: None for the renderer's.
    Returns the per-ray radiance (n, 3) in the renderer's precision.  Fed a camera's primary rays (pixel = row W + col,
    sample = s) and reduced with reduce_samples, this is render()'s linear image in mode "vectorized", bit for bit, as
    long as no ray leaves the query's |d|^2 range (stats["invalid"] counts those).
    stats: a dict that receives ray_segments, samples, kernel_ms, steps and invalid summed over the steps.
    compact: step over ray lists compacted on the device (GpuRenderer.path_step_list_into): each step runs over the
    rays the last one scattered, the host reads one 4-byte count per step and the status, directions and colour once
    at the end.  The same values bit for bit, and the same ray_segments, samples, steps and invalid, as long as
    stats["invalid"] is 0: a ray whose final status is invalid is 0 here, where the plain loop retires it as a miss."""
    if compact:
        return _loop_lists(renderer, origins, directions, pixel, sample, max_bounces, scene, seed, root2, stats)
    return _loop(renderer, origins, directions, pixel, sample, max_bounces, scene, seed, root2, stats, None)


def direct_light(renderer, origins, directions, pixel, sample, max_bounces, scene, light, intensity=(1.0, 1.0, 1.0),
                 seed=None, root2=False, stats=None):
    """path_trace plus next-event estimation towards a point light at `light` (3 numbers): at every hit one shadow
    ray from the hit point to the light through rt_query_occluded_async, and where nothing is in the way and the light
    is in front of the surface the ray's radiance gains colour * intensity * cos / r^2 (colour: the throughput after
    the hit's attenuation; cos: between the hit's normal and the light; r: the distance; shadow_rays makes the rays).  With every shadow ray
    occluded it returns path_trace's values."""
    return _loop(renderer, origins, directions, pixel, sample, max_bounces, scene, seed, root2, stats,
                 (tuple(light), tuple(intensity)))


def reduce_samples(radiance, n_pixels, spp):
    """Per-sample radiance (n_pixels spp, 3), pixel-major with the samples of a pixel in order, reduced as
    render_vectorized reduces it: ((((0 + a0) + a1) + a2) + a3) / spp with a_l the sum, from 0, over chunks j of sample
    4 j + l.  Computed in the radiance's precision, returned as float64 (n_pixels, 3) like a render's linear image."""
    r = np.asarray(radiance)
    T = r.dtype.type
    r = r.reshape(n_pixels, spp, 3)
    total = np.zeros((n_pixels, 3), dtype=r.dtype)
    for lane in range(4):
        a = np.zeros((n_pixels, 3), dtype=r.dtype)
        for s in range(lane, spp, 4):
            a = a + r[:, s]
        total = total + a
    return (total / T(spp)).astype(np.float64)
