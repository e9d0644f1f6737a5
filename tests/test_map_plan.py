"""The per-pixel-count plan (rt_progressive_map_plan, csrc/rt_progressive_plan.hpp) and GpuRenderer.adaptive's
argument checks, without a GPU: property tests on random done / target arrays through the library's host-only
entry point, and the same cases through a stand-alone AddressSanitizer + UBSan program
(tests/sanitize/map_plan_san.cpp) that includes the header alone and writes the items into a heap array of exactly
the size the plan reports."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt_mi355x as rt
from rt_mi355x import abi
from rt_mi355x.renderer import check_adaptive

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P = ctypes.POINTER(ctypes.c_uint32)
MAX_ITEMS = 0x7FFFFFFF
WAVES = [0, 1, 7, 64, 5120, 1 << 20]


def map_plan(lib, done, target, waves, capacity=None):
    """(rc, S, n_items, items [n, 4] | None): the count-only call, then the call that writes the items."""
    done, target = np.ascontiguousarray(done, np.uint32), np.ascontiguousarray(target, np.uint32)
    s, n = ctypes.c_uint32(0xDEAD), ctypes.c_uint64(0xDEAD)
    args = (len(done), done.ctypes.data_as(U32P), target.ctypes.data_as(U32P), waves, ctypes.byref(s), ctypes.byref(n))
    rc = lib.rt_progressive_map_plan(*args, None, 0)
    if rc != abi.RT_OK:
        return rc, s.value, n.value, None
    cap = n.value if capacity is None else capacity
    items = np.full((max(cap, 1), 4), 0xDEAD, np.uint32)
    rc = lib.rt_progressive_map_plan(*args, items.ctypes.data_as(U32P), cap)
    return rc, s.value, n.value, items[:cap]


def split_plan(lib, n_pixels, spp, waves):
    s, n = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.rt_split_plan(n_pixels, spp, waves, ctypes.byref(s), ctypes.byref(n)) == abi.RT_OK
    return s.value, n.value


def random_cases(seed=7, n_cases=300):
    """(done, target, waves): few and many pixels, windows of 0, 1, a few and thousands of samples, starts on and
    off the 128 grain, some pixels inactive, against few and many resident waves."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        n = int(rng.choice([1, 2, 3, 12, 144, 1000]))
        hi = int(rng.choice([4, 130, 600, 5000, 1 << 20]))
        n = min(n, 12) if hi > 5000 else n            # up to 8192 items per pixel there
        done = rng.integers(0, hi, n, dtype=np.uint32)
        if i % 3 == 0:
            done = done // 128 * 128
        length = rng.integers(0, max(2, hi // int(rng.choice([1, 4, 64]))), n, dtype=np.uint32)
        length[rng.random(n) < 0.25] = 0
        target = np.minimum(done.astype(np.uint64) + length, 1 << 20).astype(np.uint32)
        out.append((done, target, int(rng.choice(WAVES))))
    return out


def check_plan(lib, done, target, waves, S, n_items, items):
    active = target > done
    assert (items[:, 3] == 0).all()
    if not active.any():
        assert (S, n_items) == (0, 0)
        return
    mean = -(-int((target[active] - done[active]).sum()) // int(active.sum()))
    assert S == split_plan(lib, int(active.sum()), mean, waves)[0]
    pix = items[:, 0].astype(np.int64)
    assert (np.diff(pix) >= 0).all()                                   # pixel order, a pixel's items adjacent
    assert set(np.unique(pix)) == set(np.flatnonzero(active))          # every active pixel, no other
    first, end = items[:, 1].astype(np.int64), items[:, 2].astype(np.int64)
    assert (end > first).all()
    starts = np.flatnonzero(np.diff(pix, prepend=-1) != 0)             # each pixel's first item
    ends = np.append(starts[1:], len(pix)) - 1
    np.testing.assert_array_equal(first[starts], done[pix[starts]])    # the items tile [done, target) exactly once
    np.testing.assert_array_equal(end[ends], target[pix[ends]])
    inner = np.flatnonzero(np.diff(pix) == 0)
    np.testing.assert_array_equal(end[inner], first[inner + 1])
    if S % 128 == 0:
        # no two items of a pixel share a 128-byte line of its u8 e array: every inner boundary is on the grain
        assert (end[inner] % 128 == 0).all() and (end - first <= S).all()
        base = done[pix] // 128 * 128
        j = (first - base) // S
        np.testing.assert_array_equal(first, np.maximum(done[pix], base + j * S))
        np.testing.assert_array_equal(end, np.minimum(target[pix], base + (j + 1) * S))
    else:
        assert len(pix) == int(active.sum())                           # one item per active pixel
        np.testing.assert_array_equal(end - first, (target - done)[active])


def test_random_maps(lib):
    split = single = 0
    for done, target, waves in random_cases():
        rc, S, n_items, items = map_plan(lib, done, target, waves)
        assert rc == abi.RT_OK and len(items) == n_items, (rc, lib.rt_last_error())
        check_plan(lib, done, target, waves, S, n_items, items)
        split += S % 128 == 0 and n_items > int((target > done).sum())
        single += S % 128 != 0
    assert split > 20 and single > 20        # both kinds of plan were seen


def test_uniform_map_is_the_window_plan(lib):
    """Every pixel from the same done to the same target: the boundaries [max(done, base + j S), min(target,
    base + (j + 1) S)) of rt_progressive_extend_async, S from rt_split_plan over the window."""
    for n, done, target, waves in [(12, 0, 512, 5120), (12, 100, 512, 5120), (2304, 512, 4096, 5120), (3, 7, 8, 64),
                                   (144, 128, 640, 4096), (5, 129, 257, 1 << 20), (144, 8, 16, 5120), (1000, 0, 64, 64)]:
        S, _ = split_plan(lib, n, target - done, waves)
        rc, S_map, n_items, items = map_plan(lib, np.full(n, done), np.full(n, target), waves)
        assert rc == abi.RT_OK and S_map == S
        base = done - done % 128 if S % 128 == 0 else done
        nsub = -(-(target - base) // S)
        want = [(p, max(done, base + j * S), min(target, base + (j + 1) * S), 0) for p in range(n) for j in range(nsub)]
        assert n_items == n * nsub and items.tolist() == [list(w) for w in want], (n, done, target, waves)


def test_error_codes(lib):
    one, two = np.array([1], np.uint32), np.array([2], np.uint32)
    s, n = ctypes.c_uint32(), ctypes.c_uint64()
    p = lambda a: a.ctypes.data_as(U32P)   # noqa: E731

    def call(n_pix, done, target, s_out=ctypes.byref(s), n_out=ctypes.byref(n), items=None, cap=0):
        return lib.rt_progressive_map_plan(n_pix, done, target, 64, s_out, n_out, items, cap)

    assert call(1, p(one), p(two)) == abi.RT_OK and (s.value, n.value) == (1, 1)
    assert call(1, p(one), p(one)) == abi.RT_OK and (s.value, n.value) == (0, 0)          # nothing active
    for rc in (call(1, p(one), p(two), s_out=None), call(1, p(one), p(two), n_out=None), call(1, None, p(two)),
               call(1, p(one), None), call(0, p(one), p(two)), call(1, p(two), p(one))):
        assert rc == abi.RT_ERR_INVALID and b"rt_progressive_map_plan" in lib.rt_last_error()
    assert (s.value, n.value) == (0, 0)                                                   # outputs cleared
    big = np.array([(1 << 20) + 1], np.uint32)
    assert call(1, p(one), p(big)) == abi.RT_ERR_UNSUPPORTED
    assert call(1 << 31, p(one), p(two)) == abi.RT_ERR_UNSUPPORTED                        # refused before any read
    # too small an item array: refused, nothing written, the count still reported
    rc, S, n_items, items = map_plan(lib, [0, 0, 5], [300, 0, 700], 5120, capacity=2)
    assert (rc, S, n_items) == (abi.RT_ERR_INVALID, 128, 9) and (items == 0xDEAD).all()
    # more than 0x7FFFFFFF items: 262 145 pixels of 2^20 samples in items of 128
    npx = (MAX_ITEMS + 1) // 8192 + 1
    rc, S, n_items, _ = map_plan(lib, np.zeros(npx, np.uint32), np.full(npx, 1 << 20, np.uint32), 0xFFFFFFFF)
    assert rc == abi.RT_ERR_UNSUPPORTED


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_plan_under_asan_ubsan(lib, tmp_path):
    """The same cases through the stand-alone sanitizer program (the header alone, its own main): the items land
    in a heap array of exactly n_items records, a too-small one is refused untouched, and the program's plans equal
    the library's."""
    exe = str(tmp_path / "map_plan_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-o", exe, os.path.join(REPO, "tests", "sanitize", "map_plan_san.cpp")],
                   check=True)
    cases = [(d, t, w, slack) for (d, t, w), slack in zip(random_cases(seed=11, n_cases=120), [0, 0, 3, -1] * 30)]
    text = "".join(f"{len(d)} {w} {slack} " + " ".join(f"{a} {b}" for a, b in zip(d, t)) + "\n" for d, t, w, slack in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    at = 0
    for done, target, waves, slack in cases:
        rc, S, n_items = (int(x) for x in lines[at].split())
        at += 1
        rc_l, S_l, n_l, items_l = map_plan(lib, done, target, waves)
        assert (S, n_items) == (S_l, n_l) and rc_l == abi.RT_OK
        if slack < 0 and n_items > 0:
            assert rc == abi.RT_ERR_INVALID
            continue
        assert rc == abi.RT_OK
        got = np.array([ln.split() for ln in lines[at:at + n_items]], dtype=np.uint32).reshape(-1, 3)
        at += n_items
        np.testing.assert_array_equal(got, items_l[:, :3])
    assert at == len(lines)


def test_adaptive_argument_checks():
    """GpuRenderer.adaptive refuses spp_min < 1, spp_min > spp_max and a NaN tolerance before any GPU call."""
    assert check_adaptive(8, 64, 0.5) == (8, 64, 0.5) and check_adaptive(np.uint32(4), 4, 0) == (4, 4, 0.0)
    assert check_adaptive(1, 2, float("inf"))[2] == float("inf")
    for bad in ((0, 64, 0.1), (-1, 64, 0.1), (65, 64, 0.1), (8, 64, float("nan")), (8.0, 64, 0.1), (True, 64, 0.1)):
        with pytest.raises(ValueError):
            check_adaptive(*bad)
    r = rt.GpuRenderer.__new__(rt.GpuRenderer)   # no context: the checks run before any library call
    for bad in ((0, 64, 0.1), (65, 64, 0.1), (8, 64, float("nan"))):
        with pytest.raises(ValueError):
            r.adaptive(8, *bad, None, None)
    r.ctx = None
