"""ctypes binding of the test-only device library (tests/device/rt_devunit.hip ->
rust-ray-tracing_amd/lib/librt_devunit.so): the kernel's device math, one function per map kernel.

Every array is padded to a multiple of 256 (whole waves, whole blocks) with a value inside the function's
fast-path contract, so the wave ballots inside dvs / sqrt_len see only inputs the caller chose; pad() is the
same padding, for the CPU tests that check the contract per wave.  Vectors are [3, n], component-major.
RT_DEVUNIT_LIB names another build (the mutation check).
"""
import ctypes
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rust-ray-tracing_amd")
DEVUNIT_PATH = os.path.join(PKG, "lib", "librt_devunit.so")
BLOCK = 256
WAVE = 64
SLOTS = 8

_lib = None


def load_devunit():
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RT_DEVUNIT_LIB", DEVUNIT_PATH)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C {PKG} devunit`")
    lib = ctypes.CDLL(path)
    vp, sz, u32, u64, f64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    for sfx in ("f32", "f64"):
        for name, args in (("unit", [vp, vp, sz]), ("dvs", [vp, vp, vp, sz]), ("sqrt_nd", [vp, vp, sz]),
                           ("sqrt_len", [vp, vp, sz]), ("sincos2pi", [vp, vp, vp, sz]), ("unit_vec", [vp, vp, vp, sz]),
                           ("refract", [vp, vp, vp, vp, sz]), ("q8", [vp, vp, sz]), ("div_dim", [vp, u32, f64, vp, sz]),
                           ("rng", [vp, vp, vp, vp, u32, u32, vp, vp, vp, sz]),
                           ("hit", [vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, sz])):
            fn = getattr(lib, f"du_{name}_{sfx}")
            fn.argtypes, fn.restype = args, ctypes.c_int
        for name, third in (("probe_general", vp), ("probe_camera", vp)):
            fn = getattr(lib, f"du_{name}_{sfx}")
            fn.argtypes, fn.restype = [vp, ctypes.c_int, ctypes.c_int, third, vp, vp, vp, vp, sz], ctypes.c_int
        fn = getattr(lib, f"du_next_ray_{sfx}")
        fn.argtypes, fn.restype = [vp, vp, u64, ctypes.c_int] + [vp] * 11 + [sz], ctypes.c_int
    lib.du_scene_layout.argtypes, lib.du_scene_layout.restype = [vp, vp, vp, sz], ctypes.c_int
    lib.du_philox4x32_10.argtypes = lib.du_philox2x32_10.argtypes = [vp, vp, vp, sz]
    lib.du_fold_key_f32.argtypes, lib.du_fold_key_f32.restype = [u64], u32
    lib.du_sqrt_sweep_f32.argtypes = [u32, u64, ctypes.c_int, ctypes.POINTER(u64), vp]
    _lib = lib
    return lib


def pad(a, fill):
    """a ([n] or [k, n]) padded along the last axis to a multiple of BLOCK with `fill`, contiguous."""
    a = np.asarray(a)
    n = a.shape[-1]
    m = -(-n // BLOCK) * BLOCK
    out = np.full(a.shape[:-1] + (m,), fill, dtype=a.dtype)
    out[..., :n] = a
    return out


def _sfx(dtype):
    return {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[np.dtype(dtype)]


def _call(name, dtype, *args):
    rc = getattr(load_devunit(), f"du_{name}_{_sfx(dtype)}" if dtype is not None else f"du_{name}")(*args)
    if rc != 0:
        raise RuntimeError(f"du_{name}: HIP error {rc}")


def _p(a):
    return a.ctypes.data


def unit(v):
    n, vp = v.shape[1], pad(v, 1.0)
    out = np.empty_like(vp)
    _call("unit", v.dtype, _p(vp), _p(out), vp.shape[1])
    return out[:, :n]


def dvs(v, s):
    n, vp, sp = v.shape[1], pad(v, 1.0), pad(s, 1.0)
    out = np.empty_like(vp)
    _call("dvs", v.dtype, _p(vp), _p(sp), _p(out), vp.shape[1])
    return out[:, :n]


def _map1(name, x, fill=1.0, out_dtype=None):
    n, xp = x.size, pad(x, fill)
    out = np.empty(xp.size, out_dtype or x.dtype)
    _call(name, x.dtype, _p(xp), _p(out), xp.size)
    return out[:n]


def sqrt_nd(x):
    return _map1("sqrt_nd", x)


def sqrt_len(x):
    return _map1("sqrt_len", x)


def q8(v):
    return _map1("q8", v, out_dtype=np.uint8)


def sincos2pi(u):
    n, up = u.size, pad(u, 0.25)
    s, c = np.empty_like(up), np.empty_like(up)
    _call("sincos2pi", u.dtype, _p(up), _p(s), _p(c), up.size)
    return s[:n], c[:n]


def unit_vec(u1, u2):
    n, a, b = u1.size, pad(u1, 0.25), pad(u2, 0.25)
    out = np.empty((3, a.size), u1.dtype)
    _call("unit_vec", u1.dtype, _p(a), _p(b), _p(out), a.size)
    return out[:, :n]


def refract(v, nrm, ratio):
    n, a, b, r = v.shape[1], pad(v, 1.0), pad(nrm, 1.0), pad(ratio, 1.0)
    out = np.empty_like(a)
    _call("refract", v.dtype, _p(a), _p(b), _p(r), _p(out), a.shape[1])
    return out[:, :n]


def div_dim(x, W, r):
    n, xp = x.size, pad(x, 0.0)
    out = np.empty_like(xp)
    _call("div_dim", x.dtype, _p(xp), int(W), float(r), _p(out), xp.size)
    return out[:n]


def fold_key_f32(seed):
    return int(load_devunit().du_fold_key_f32(seed))


def rng(dtype, sid, pix, k, stream, seed):
    """rng<T> + u01a / u01b with the key the host derives from the 64-bit seed (fp32: folded).
    Returns (block [4, n] u32, ua, ub); fp32 fills block rows 2, 3 with zero."""
    n = len(sid)
    a = [pad(np.asarray(x, np.uint32), 0) for x in (sid, pix, k, stream)]
    m = a[0].size
    r, ua, ub = np.empty((4, m), np.uint32), np.empty(m, dtype), np.empty(m, dtype)
    if np.dtype(dtype) == np.float32:
        k0, k1 = fold_key_f32(seed), 0
    else:
        k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    _call("rng", dtype, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), k0, k1, _p(r), _p(ua), _p(ub), m)
    return r[:, :n], ua[:n], ub[:n]


def philox4x32_10(ctr, key):
    """ctr [4, n], key [2, n] -> [4, n]."""
    n, c, k = ctr.shape[1], pad(np.asarray(ctr, np.uint32), 0), pad(np.asarray(key, np.uint32), 0)
    out = np.empty_like(c)
    _call("philox4x32_10", None, _p(c), _p(k), _p(out), c.shape[1])
    return out[:, :n]


def philox2x32_10(ctr, key):
    """ctr [2, n], key [n] -> [2, n]."""
    n, c, k = ctr.shape[1], pad(np.asarray(ctr, np.uint32), 0), pad(np.asarray(key, np.uint32), 0)
    out = np.empty_like(c)
    _call("philox2x32_10", None, _p(c), _p(k), _p(out), c.shape[1])
    return out[:, :n]


HIT_MODES = {"packed": 0, "root2": 1, "scalar": 2}


def hit(hb, disc, idx, cnt, a, mode):
    """hit_update<T, root2, SCALAR> folded over each lane's first cnt (<= 8) candidates (hb, disc, idx: [8, n]).
    Returns (bt [n], bi [n] int32).  Padding lanes hold no candidate."""
    n = hb.shape[1]
    h, d, a_ = pad(hb, 1.0), pad(disc, 1.0), pad(a, 1.0)
    i, c = pad(np.asarray(idx, np.uint32), 0), pad(np.asarray(cnt, np.uint32), 0)
    t, bi = np.empty(h.shape[1], hb.dtype), np.empty(h.shape[1], np.int32)
    _call("hit", hb.dtype, _p(h), _p(d), _p(i), _p(c), _p(a_), HIT_MODES[mode], _p(t), _p(bi), h.shape[1])
    return t[:n], bi[:n]


def sqrt_sweep_f32(start, count, mode):
    """sqrt over `count` consecutive fp32 bit patterns from `start`, compared on the device with (float)sqrt((double)x).
    mode 0: sqrt_len; 1: sqrt_len, lane 7 of every odd wave replaced by a tiny positive argument; 2: sqrt_nd.
    Returns (mismatches, the first up to 16 offending bit patterns)."""
    mis = ctypes.c_uint64(0)
    first = np.zeros(16, np.uint32)
    rc = load_devunit().du_sqrt_sweep_f32(start, count, mode, ctypes.byref(mis), _p(first))
    if rc != 0:
        raise RuntimeError(f"du_sqrt_sweep_f32: HIP error {rc}")
    return mis.value, first[:min(mis.value, 16)]


# ---- the ray probe: the product's sweeps on chosen rays (tests/test_gpu_cull_probe.py) ----
PROBE_MODES = {"packed": 0, "root2": 1, "scalar": 2}
IDX_UNTOUCHED = -7          # what an inactive lane's outputs hold before and after a probe
T_UNTOUCHED = -12345.0


def scene_layout(flat):
    """build_scene_image's counts and slot -> scene index table of a FlatScene (host only: no GPU).
    Returns (dict of n_xg, n_xs, n_top, n_mg, n_gg, n_supc; ridx [4 n_xg + 16 clusters] uint32, 0xFFFFFFFF: dummy)."""
    lib = load_devunit()
    counts = np.zeros(8, np.uint32)
    rc = lib.du_scene_layout(ctypes.addressof(flat.abi), _p(counts), None, 0)
    assert rc == 0, rc
    ridx = np.zeros(int(counts[6]), np.uint32)
    rc = lib.du_scene_layout(ctypes.addressof(flat.abi), _p(counts), _p(ridx), ridx.size)
    assert rc == 0, rc
    names = ("n_xg", "n_xs", "n_top", "n_mg", "n_gg", "n_supc")
    return {k: int(v) for k, v in zip(names, counts)}, ridx[:4 * int(counts[0]) + 64 * int(counts[2])]


def _probe(name, flat, mode, filter_off, first, d, active):
    d = np.ascontiguousarray(d)
    n = d.shape[1]
    assert n % BLOCK == 0 and d.shape == (3, n) and first.dtype == d.dtype
    active = np.ascontiguousarray(active, np.uint8)
    assert active.shape == (n,)
    idx = np.full(n, IDX_UNTOUCHED, np.int32)
    t = np.full(n, T_UNTOUCHED, d.dtype)
    _call(name, d.dtype, ctypes.addressof(flat.abi), PROBE_MODES[mode], int(bool(filter_off)), _p(first), _p(d),
          _p(active), _p(idx), _p(t), n)
    return idx, t


def probe_general(flat, mode, o, d, active, filter_off=False):
    """nearest_hit<T, ROOT2, SCALAR, MEGA> for the active lanes of n rays (o, d: [3, n], n a multiple of 256;
    lane i of the launch holds ray i).  Returns (idx [n] int32, t [n]); -1 / +inf: no hit; inactive lanes hold
    IDX_UNTOUCHED / T_UNTOUCHED."""
    o = np.ascontiguousarray(o)
    assert o.shape == d.shape
    return _probe("probe_general", flat, mode, filter_off, o, d, active)


def probe_camera(flat, mode, centre, d, active, filter_off=False):
    """camera_sweep<T, ROOT2, SCALAR, MEGA>(active, d) per wave, over build_cam_table's tables for `centre` [3]."""
    centre = np.ascontiguousarray(centre, d.dtype)
    assert centre.shape == (3,)
    return _probe("probe_camera", flat, mode, filter_off, centre, d, active)


# ---- the next-ray probe: the product's next_ray<T, SCALAR> on chosen lanes (tests/test_gpu_scatter.py) ----
NEXT_RAY_MODES = {"packed": 0, "scalar": 1}
ROLE_IDLE, ROLE_CAMERA, ROLE_SCATTER = 0, 1, 2


def next_ray(flat, cam, seed, mode, role, colx, rowy, pix, sid, k, hit_i, hit_t, o, d, c):
    """next_ray<T, SCALAR> per lane (n a multiple of 256; lane i of the launch holds entry i), over the kernel
    arguments the product's host steps make of (flat, cam, seed).  role [n] u8: ROLE_IDLE (does not enter),
    ROLE_CAMERA (colx, rowy, pix, sid), ROLE_SCATTER (o, d, c, hit_i, hit_t, k, pix, sid).  o, d, c: [3, n], float32 or
    float64 picks the build.  Returns new (o, d, c); an idle lane's are the caller's."""
    dt = o.dtype
    o, d, c = (np.array(a, dtype=dt, order="C", copy=True) for a in (o, d, c))
    n = o.shape[1]
    assert n % BLOCK == 0 and o.shape == d.shape == c.shape == (3, n)
    role = np.ascontiguousarray(role, np.uint8)
    colx, rowy, pix, sid, k = (np.ascontiguousarray(a, np.uint32) for a in (colx, rowy, pix, sid, k))
    hit_i, hit_t = np.ascontiguousarray(hit_i, np.int32), np.ascontiguousarray(hit_t, dt)
    assert all(a.shape == (n,) for a in (role, colx, rowy, pix, sid, k, hit_i, hit_t))
    _call("next_ray", dt, ctypes.addressof(flat.abi), ctypes.addressof(cam), seed, NEXT_RAY_MODES[mode], _p(role), _p(colx),
          _p(rowy), _p(pix), _p(sid), _p(k), _p(hit_i), _p(hit_t), _p(o), _p(d), _p(c), n)
    return o, d, c
