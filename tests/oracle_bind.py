"""ctypes binding of the test-only oracle (oracle/build/liboracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use this module.
"""
import ctypes
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
ORACLE_PATH = os.path.join(ORACLE_DIR, "build", "liboracle.so")

NATIVE_PATH = os.path.join(ORACLE_DIR, "build", "native", "liboracle.so")

_libs = {}


def build_native():
    """Build the -march=native oracle on this host (bench.py's CPU baseline); returns its path or None."""
    r = subprocess.run(["make", "-C", ORACLE_DIR, "native"], capture_output=True, text=True)
    return NATIVE_PATH if r.returncode == 0 and os.path.exists(NATIVE_PATH) else None


def load_oracle(path=None):
    path = path or ORACLE_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ORACLE_DIR], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    vp, u32, u64, f64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    for name in ("oracle_render_f64", "oracle_render_f32"):
        fn = getattr(lib, name)
        fn.argtypes = [vp, vp, u32, u32, u64, u32, vp, u32, vp, vp, ctypes.POINTER(u64), ctypes.c_int]
        fn.restype = ctypes.c_int
    lib.oracle_camera_new.argtypes = [vp, u32, u32, f64, f64, ctypes.POINTER(f64), ctypes.POINTER(f64),
                                      ctypes.POINTER(f64), f64]
    lib.oracle_philox4x32_10.argtypes = [ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.oracle_philox2x32_10.argtypes = [ctypes.POINTER(u32), u32, ctypes.POINTER(u32)]
    lib.oracle_sincos2pi_f64.argtypes = [f64, ctypes.POINTER(f64), ctypes.POINTER(f64)]
    lib.oracle_to_u8.argtypes = [ctypes.POINTER(f64), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int)]
    lib.oracle_get_ray_f64.argtypes = [vp, u32, u32, u32, u64, ctypes.POINTER(f64), ctypes.POINTER(f64)]
    sz = ctypes.c_size_t
    for sfx in ("f64", "f32"):
        getattr(lib, f"oracle_sincos2pi_{sfx}_n").argtypes = [vp, vp, vp, sz]
        getattr(lib, f"oracle_unit_vec_{sfx}_n").argtypes = [vp, vp, vp, sz]
        getattr(lib, f"oracle_unit_{sfx}_n").argtypes = [vp, vp, sz]
        getattr(lib, f"oracle_refract_{sfx}_n").argtypes = [vp, vp, vp, vp, sz]
        getattr(lib, f"oracle_q8_{sfx}_n").argtypes = [vp, vp, sz]
        getattr(lib, f"oracle_draw_{sfx}_n").argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, sz]
        for name in ("sincos2pi", "unit_vec", "unit", "refract", "q8", "draw"):
            getattr(lib, f"oracle_{name}_{sfx}_n").restype = None
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"oracle_nearest_hit_{sfx}")
        fn.argtypes, fn.restype = [vp, u32, sz, vp, vp, vp, vp], ctypes.c_int
        fn = getattr(lib, f"oracle_next_ray_{sfx}_n")
        fn.argtypes, fn.restype = [vp, u64, u32, sz] + [vp] * 14, ctypes.c_int
        fn = getattr(lib, f"oracle_get_ray_{sfx}_n")
        fn.argtypes, fn.restype = [vp, u64, sz] + [vp] * 6, ctypes.c_int
    lib.oracle_fmix32.argtypes = [u32]
    lib.oracle_fmix32.restype = u32
    _libs[path] = lib
    return lib


# ---- batched probes (oracle.h ORACLE_PROBE_DECLS): numpy in, numpy out; dtype float32 or float64 picks the build ----
def _sfx(dtype):
    return {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[np.dtype(dtype)]


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def oracle_sincos2pi(u):
    u = _c(u, u.dtype)
    s, c = np.empty_like(u), np.empty_like(u)
    getattr(load_oracle(), f"oracle_sincos2pi_{_sfx(u.dtype)}_n")(u.ctypes.data, s.ctypes.data, c.ctypes.data, u.size)
    return s, c


def oracle_unit_vec(u1, u2):
    u1, u2 = _c(u1, u1.dtype), _c(u2, u1.dtype)
    out = np.empty((3, u1.size), u1.dtype)
    getattr(load_oracle(), f"oracle_unit_vec_{_sfx(u1.dtype)}_n")(u1.ctypes.data, u2.ctypes.data, out.ctypes.data, u1.size)
    return out


def oracle_unit(v):
    """v: [3, n] component-major."""
    v = _c(v, v.dtype)
    out = np.empty_like(v)
    getattr(load_oracle(), f"oracle_unit_{_sfx(v.dtype)}_n")(v.ctypes.data, out.ctypes.data, v.shape[1])
    return out


def oracle_refract(v, n, ratio):
    v, n, ratio = _c(v, v.dtype), _c(n, v.dtype), _c(ratio, v.dtype)
    out = np.empty_like(v)
    getattr(load_oracle(), f"oracle_refract_{_sfx(v.dtype)}_n")(v.ctypes.data, n.ctypes.data, ratio.ctypes.data,
                                                                 out.ctypes.data, v.shape[1])
    return out


def oracle_q8(v):
    v = _c(v, v.dtype)
    out = np.empty(v.size, np.uint8)
    getattr(load_oracle(), f"oracle_q8_{_sfx(v.dtype)}_n")(v.ctypes.data, out.ctypes.data, v.size)
    return out


def oracle_draw(dtype, sid, pix, k, stream, seed):
    """draw + u01 / u01b for the 64-bit seed: (block [4, n] u32, ua, ub)."""
    sid, pix, k, stream = (_c(a, np.uint32) for a in (sid, pix, k, stream))
    n = sid.size
    r = np.empty((4, n), np.uint32)
    ua, ub = np.empty(n, dtype), np.empty(n, dtype)
    getattr(load_oracle(), f"oracle_draw_{_sfx(dtype)}_n")(sid.ctypes.data, pix.ctypes.data, k.ctypes.data, stream.ctypes.data,
                                                            seed & 0xFFFFFFFF, seed >> 32, r.ctypes.data, ua.ctypes.data,
                                                            ub.ctypes.data, n)
    return r, ua, ub


NEAREST_MODES = {"packed": 0, "root2": 1, "scalar": 2}


def oracle_nearest_hit(flat, mode, o, d):
    """The nearest hit of each ray (o, d: [3, n], float32 or float64 picks the build), brute force over every sphere
    of flat in scene order.  mode: "packed" (hit_packed + update, Q1), "root2" or "scalar".
    Returns (idx [n] int32, -1 for no hit; t [n], +inf for no hit)."""
    o = _c(o, o.dtype)
    d = _c(d, o.dtype)
    n = o.shape[1]
    assert o.shape == d.shape == (3, n)
    idx, t = np.empty(n, np.int32), np.empty(n, o.dtype)
    rc = getattr(load_oracle(), f"oracle_nearest_hit_{_sfx(o.dtype)}")(ctypes.addressof(flat.abi), NEAREST_MODES[mode], n,
                                                                       o.ctypes.data, d.ctypes.data, idx.ctypes.data,
                                                                       t.ctypes.data)
    assert rc == 0, rc
    return idx, t


NEXT_RAY_MODES = {"packed": 0, "scalar": 1}
BRANCHES = ("lambertian", "near_zero", "metal", "cannot_refract", "schlick_reflect", "refract")   # OR_BRANCH_*


def oracle_next_ray(flat, seed, mode, o, d, hit_i, hit_t, sid, pix, k, colour):
    """What follows a hit, per lane (oracle.h oracle_next_ray_*_n): o, d, colour [3, n] (float32 or float64 picks the
    build), hit_i, hit_t, sid, pix, k [n].  mode: "packed" or "scalar".
    Returns (o' [3, n], d' [3, n], colour' [3, n], normal [3, n], front [n] u8, code [n] u8: index into BRANCHES)."""
    o = _c(o, o.dtype)
    dt = o.dtype
    d, colour, hit_t = _c(d, dt), _c(colour, dt), _c(hit_t, dt)
    hit_i = _c(hit_i, np.int32)
    sid, pix, k = (_c(a, np.uint32) for a in (sid, pix, k))
    n = o.shape[1]
    assert o.shape == d.shape == colour.shape == (3, n) and all(a.shape == (n,) for a in (hit_i, hit_t, sid, pix, k))
    oo, do, co, nrm = (np.empty((3, n), dt) for _ in range(4))
    front, code = np.empty(n, np.uint8), np.empty(n, np.uint8)
    rc = getattr(load_oracle(), f"oracle_next_ray_{_sfx(dt)}_n")(
        ctypes.addressof(flat.abi), seed, NEXT_RAY_MODES[mode], n, o.ctypes.data, d.ctypes.data, hit_i.ctypes.data,
        hit_t.ctypes.data, sid.ctypes.data, pix.ctypes.data, k.ctypes.data, colour.ctypes.data, oo.ctypes.data,
        do.ctypes.data, co.ctypes.data, nrm.ctypes.data, front.ctypes.data, code.ctypes.data)
    assert rc == 0, rc
    return oo, do, co, nrm, front, code


def oracle_get_ray(dtype, cam, seed, col, row, pix, sid):
    """Camera::get_ray per lane (cam: abi.RtCamera): (o [3, n], d [3, n]) in dtype."""
    col, row, pix, sid = (_c(a, np.uint32) for a in (col, row, pix, sid))
    n = col.size
    o, d = np.empty((3, n), dtype), np.empty((3, n), dtype)
    rc = getattr(load_oracle(), f"oracle_get_ray_{_sfx(dtype)}_n")(ctypes.addressof(cam), seed, n, col.ctypes.data,
                                                                   row.ctypes.data, pix.ctypes.data, sid.ctypes.data,
                                                                   o.ctypes.data, d.ctypes.data)
    assert rc == 0, rc
    return o, d


def oracle_render(flat, cam, max_bounces, spp, seed, flags=0, pixels=None, precision="f64", threads=None,
                  lib_path=None):
    """Run the CPU restatement.  flat: rt_mi355x.FlatScene; cam: abi.RtCamera.
    Returns (rgb [n,3] u8, linear [n,3] f64, segments, rc)."""
    lib = load_oracle(lib_path)
    if threads is None:
        threads = min(16, os.cpu_count() or 1)
    if pixels is None:
        n = cam.image_width * cam.image_height
        pix_ptr = None
    else:
        pixels = np.ascontiguousarray(pixels, dtype=np.uint32)
        n = len(pixels)
        pix_ptr = pixels.ctypes.data
    rgb = np.zeros((n, 3), dtype=np.uint8)
    lin = np.zeros((n, 3), dtype=np.float64)
    segs = ctypes.c_uint64(0)
    fn = lib.oracle_render_f64 if precision == "f64" else lib.oracle_render_f32
    rc = fn(ctypes.addressof(flat.abi), ctypes.addressof(cam), max_bounces, spp, seed, flags, pix_ptr, n,
            rgb.ctypes.data, lin.ctypes.data, ctypes.byref(segs), threads)
    return rgb, lin, segs.value, rc


def packed_render(flat, cam, max_bounces, spp, seed, tiles=None, tile=128, threads=None, lib_path=None):
    """The reference-shaped CPU baseline (oracle/packed_avx2.h, f64): 4-lane AVX2 packets, tile x tile
    blocks through a shared queue.  tiles: block indices (row-major block grid) or None = all.
    Returns (rgb [W*H,3] u8, linear [W*H,3] f64 -- only the rendered blocks written, segments, pixels, rc)."""
    lib = load_oracle(lib_path)
    fn = lib.packed_render_f64
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    fn.argtypes = [vp, vp, u32, u32, u64, u32, vp, u32, vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.c_int]
    fn.restype = ctypes.c_int
    if threads is None:
        threads = min(16, os.cpu_count() or 1)
    n = cam.image_width * cam.image_height
    rgb = np.zeros((n, 3), dtype=np.uint8)
    lin = np.zeros((n, 3), dtype=np.float64)
    tptr, nt = None, 0
    if tiles is not None:
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
        tptr, nt = tiles.ctypes.data, len(tiles)
    segs, pix = u64(0), u64(0)
    rc = fn(ctypes.addressof(flat.abi), ctypes.addressof(cam), max_bounces, spp, seed, tile, tptr, nt,
            rgb.ctypes.data, lin.ctypes.data, ctypes.byref(segs), ctypes.byref(pix), threads)
    return rgb, lin, segs.value, pix.value, rc
