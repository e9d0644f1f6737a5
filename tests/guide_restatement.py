"""The guide buffers' definition (include/rt_mi355x.h) restated on tests/independent_v2.py, shared by
tests/test_gpu_guides.py, tests/test_gpu_guide_edges.py (GPU: guide_pixels<T, CAMQ, MEGA> against it), tests/test_guide_edges.py
and tests/test_guides_abi.py (CPU).

Plain module: no GPU, no fixtures.  independent_v2 is imported, not modified: get_ray gives the primary ray of
(pixel, sample, seed), hit_scene the live path's closest hit at bounce 0 with the finalized normal,
scene_from_flat the materials in the render's precision, and fold() is the definition's reduction in numpy.
Per-sample values do not depend on the sample count, so each frame's samples are restated once, at the largest
count a test needs, and every smaller count folds a prefix of them.
"""
import numpy as np

import independent_v2 as iv
from rt_mi355x import abi

SEED = 0x5EED0001


def fold(vals):
    """The definition's reduction of one channel's per-sample values (doubles) to the float32 output."""
    vals = np.asarray(vals, dtype=np.float64)
    n = len(vals)
    p = np.zeros(64)
    for s, v in enumerate(vals):
        p[s % 64] += v
    h = 32
    while h:
        p[:h] += p[h:2 * h]
        h //= 2
    return np.float32(p[0] / float(n))


def cam_dict(cam):
    """independent_v2's camera from the rt_camera the library gets (the same doubles)."""
    return {"W": cam.image_width, "H": cam.image_height, "center": tuple(cam.center), "ulc": tuple(cam.ulc),
            "vu": tuple(cam.vu), "vv": tuple(cam.vv), "du": tuple(cam.du), "dv": tuple(cam.dv)}


def restate_samples(flat, cam, spp, prec, pixels=None, seed=SEED):
    """Per pixel (global indices; None: the whole frame) and sample s < spp: the eight per-sample values
    (albedo r g b, normal x y z, depth, coverage) as doubles [P, spp, 8], and the hit sphere (-1: a miss) [P, spp]."""
    spheres, smat, mats = iv.scene_from_flat(flat, prec)
    camp = iv.camera_in(cam_dict(cam), prec)
    W = cam.image_width
    pixels = range(W * cam.image_height) if pixels is None else [int(p) for p in pixels]
    vals = np.zeros((len(pixels), spp, 8))
    idx = np.full((len(pixels), spp), -1, dtype=np.int64)
    for k, pix in enumerate(pixels):
        col, row = pix % W, pix // W
        for s in range(spp):
            o, d = iv.get_ray(camp, col, row, s, pix, seed, prec)
            rec = iv.hit_scene(spheres, o, d)
            if rec is None:
                vals[k, s] = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
                continue
            t, _, n, _, i = rec
            m = mats[smat[i]]
            alb = (1.0, 1.0, 1.0) if m.kind == abi.RT_DIELECTRIC else m.albedo
            vals[k, s] = tuple(float(x) for x in alb) + tuple(float(x) for x in n) + (float(t), 1.0)
            idx[k, s] = i
    vals.setflags(write=False)
    idx.setflags(write=False)
    return vals, idx


def restate_guides(vals, spp):
    """The four outputs at spp samples from the per-sample values of at least spp samples."""
    P = vals.shape[0]
    ch = np.array([[fold(vals[k, :spp, c]) for c in range(8)] for k in range(P)], dtype=np.float32).reshape(P, 8)
    return {"albedo": ch[:, 0:3], "normal": ch[:, 3:6], "depth": ch[:, 6], "coverage": ch[:, 7]}


_refs = {}


def samples_once(key, *args, **kw):
    """restate_samples computed once per key and left unchanged."""
    if key not in _refs:
        _refs[key] = restate_samples(*args, **kw)
    return _refs[key]
