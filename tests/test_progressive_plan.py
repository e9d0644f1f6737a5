"""A progressive session's host side (csrc/rt_progressive_plan.hpp, rt_progressive_bytes in the C ABI, the
Python schedule check), on the CPU: no GPU here.

The record bytes are checked through the library (ctypes); the sample windows of an extend through a
stand-alone AddressSanitizer + UBSan program (tests/sanitize/progressive_plan_san.cpp) that includes the same
header and asserts that the items of every window tile [done, spp_total) exactly once."""
import ctypes
import itertools
import os
import subprocess

import pytest

import rt_mi355x as rt
from rt_mi355x import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = abi.RT_FLAG_F32
MAX_ITEMS = 0x7FFFFFFF


def nbytes(lib, n_pixels, cap, depth, flags):
    b = ctypes.c_uint64(0xDEAD)
    rc = lib.rt_progressive_bytes(n_pixels, cap, depth, flags, ctypes.byref(b))
    return rc, b.value


def test_full_hd_512(lib):
    """17 B per sample of capacity in fp32, 33 B in fp64: 18.0 and 35.0 GB for 1920x1080 x 512."""
    assert nbytes(lib, 1920 * 1080, 512, 50, F32) == (abi.RT_OK, 18_048_614_400)
    assert nbytes(lib, 1920 * 1080, 512, 50, 0) == (abi.RT_OK, 35_035_545_600)


def test_region_layout(lib):
    """A region is y, c (3 T) and e per position of 4 ceil(cap / 4), rounded up to 256 bytes; e is u8 up to
    depth 254 and u32 from 255."""
    for cap, depth, flags in itertools.product((1, 6, 100, 512, 4096, 70001, 1 << 20), (0, 50, 254, 255, 300), (0, F32)):
        P = 4 * ((cap + 3) // 4)
        per = 4 * (4 if flags else 8) + (4 if depth > 254 else 1)
        want = (P * per + 255) // 256 * 256
        assert nbytes(lib, 1, cap, depth, flags) == (abi.RT_OK, want), (cap, depth, flags)
        assert nbytes(lib, 77, cap, depth, flags) == (abi.RT_OK, 77 * want)
    assert nbytes(lib, 1, 512, 254, F32)[1] == 512 * 17 and nbytes(lib, 1, 512, 255, F32)[1] == 512 * 20
    assert nbytes(lib, 1, 512, 254, 0)[1] == 512 * 33 and nbytes(lib, 1, 512, 255, 0)[1] == 512 * 36
    # the limits multiply without overflow
    assert nbytes(lib, MAX_ITEMS, 1 << 20, 300, 0) == (abi.RT_OK, MAX_ITEMS * (1 << 20) * 36)


def test_bytes_refusals(lib):
    assert lib.rt_progressive_bytes(1, 1, 50, 0, None) == abi.RT_ERR_INVALID
    assert b"rt_progressive_bytes" in lib.rt_last_error()
    assert nbytes(lib, 0, 16, 50, 0) == (abi.RT_ERR_INVALID, 0)
    assert nbytes(lib, 16, 0, 50, 0) == (abi.RT_ERR_INVALID, 0)
    assert nbytes(lib, 16, (1 << 20) + 1, 50, 0) == (abi.RT_ERR_UNSUPPORTED, 0)
    assert nbytes(lib, 1 << 31, 16, 50, 0) == (abi.RT_ERR_UNSUPPORTED, 0)
    for flags in (abi.RT_FLAG_ROOT2, abi.RT_FLAG_ROOT2 | F32, abi.RT_FLAG_MODE_VECTORIZED, abi.RT_FLAG_MODE_SCALAR,
                  abi.RT_FLAG_MODE_VECTORIZED3):
        assert nbytes(lib, 16, 16, 50, flags) == (abi.RT_ERR_UNSUPPORTED, 0), flags
    assert nbytes(lib, 16, 16, 50, 0x20) == (abi.RT_ERR_INVALID, 0)   # no such flag, as in rt_render_split_async


def test_entry_points_are_exported(lib):
    names = {"rt_progressive_bytes", "rt_progressive_begin", "rt_progressive_extend_async", "rt_progressive_end"}
    assert names <= set(abi.EXPORTED)
    for name in names:
        assert hasattr(lib, name)
    assert os.path.join(abi.PKG_DIR, "csrc", "rt_progressive_plan.hpp") in abi.SOURCE_FILES
    assert hasattr(rt, "ProgressiveSession") and hasattr(rt.GpuRenderer, "begin_progressive")


class NoGpu:
    """A GpuRenderer that was never constructed: any use of the context or the library raises."""

    def __getattr__(self, name):
        raise AssertionError(f"the schedule check touched the renderer ({name})")


@pytest.mark.parametrize("schedule", [[], [16, 16], [64, 16], [16, 64, 64], [0, 16], [-4, 8], [16, 32.0], [True, 4], ["16"],
                                      iter(())])
def test_schedule_is_checked_before_any_gpu_call(schedule):
    """GpuRenderer.progressive raises ValueError on an empty or non-increasing schedule when it is called, not
    at the first next(), and without a context."""
    with pytest.raises(ValueError):
        rt.GpuRenderer.progressive(NoGpu(), 8, schedule, None, None)


def test_schedule_accepted():
    from rt_mi355x.renderer import check_schedule
    import numpy as np
    assert check_schedule([1]) == [1]
    assert check_schedule((16, 64, 1024)) == [16, 64, 1024]
    assert check_schedule(np.array([2, 4, 8])) == [2, 4, 8]
    assert check_schedule(n for n in (1, 2, 3)) == [1, 2, 3]


CLI = os.path.join(REPO, "rust-ray-tracing_amd", "bin", "rt-render")


@pytest.mark.parametrize("args,why", [
    (["--progressive", "16,64", "--spp", "1024", "--root2"], "--root2"),
    (["--progressive", "16,64", "--spp", "1024", "--mode", "scalar"], "--mode vectorized2"),
    (["--progressive", "16,64", "--spp", "1024", "--mode", "vectorized3"], "--mode vectorized2"),
    (["--progressive", "16,64", "--spp", "1024", "--block-size", "128"], "--block-size"),
    (["--progressive", "64,16", "--spp", "1024"], "strictly increasing"),
    (["--progressive", "16,16", "--spp", "1024"], "strictly increasing"),
    (["--progressive", "16,1024", "--spp", "1024"], "below --spp"),
    (["--progressive", "0,16", "--spp", "1024"], "0"),
    (["--progressive", "16,x", "--spp", "1024"], "not a sample count"),
    (["--progressive", "16,", "--spp", "1024"], "n1,n2"),
])
def test_cli_refuses_a_bad_progressive_run(tmp_path, args, why):
    """rt-render --progressive with --root2, another --mode or a bad list of counts: exit status 2 and a line
    that says why, before the scene is read or a GPU touched (there is no scene.toml in the working directory)."""
    r = subprocess.run([CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert r.stderr.startswith("--progressive: ") and why in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

DONE = [0, 1, 6, 7, 63, 64, 100, 127, 128, 129, 512, 4095, 70000, (1 << 20) - 1]
TOTAL = [1, 6, 7, 100, 128, 129, 512, 513, 4096, 70001, 1 << 20]
ITEM = [0, 1, 7, 100, 128, 256, 4736, 1 << 20]      # 0: the session's own plan
PIXELS = [1, 2, 12, 2304, 10 ** 6, MAX_ITEMS]
WAVES = [0, 4096, 5120]


def window_cases():
    cases = []
    for np_, d, t, s in itertools.product(PIXELS, DONE, TOTAL, ITEM):
        if t <= d:
            continue
        for w in (WAVES if s == 0 else [0]):
            cases.append((np_, d, t, s, w))
    # refusals: an empty or backward window, no pixels, past the limits
    cases += [(4, 16, 16, 0, 5120), (4, 17, 16, 128, 0), (0, 0, 16, 0, 5120), (4, 0, (1 << 20) + 1, 0, 5120),
              (1 << 31, 0, 16, 0, 5120), (4, 0, 16, (1 << 20) + 1, 0), (MAX_ITEMS, 0, 1 << 20, 1, 0)]
    return cases


def test_windows_under_asan_ubsan(tmp_path):
    """The items of a window tile [done, spp_total) exactly once, with no overflow: checked inside the
    stand-alone program for every case (it exits non-zero on a violation) and again here from its output."""
    exe = str(tmp_path / "progressive_plan_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-o", exe,
                    os.path.join(REPO, "tests", "sanitize", "progressive_plan_san.cpp")], check=True)
    cases = window_cases()
    text = "\n".join(" ".join(str(v) for v in c) for c in cases) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    ok = split = 0
    for case, line in zip(cases, lines):
        np_, d, t, s, w = case
        rc, S, nsub, base, n_items = (int(x) for x in line.split())
        if rc != abi.RT_OK:
            assert (S, nsub, base, n_items) == (0, 0, 0, 0), case
            # inside the limits the only refusal is more items than one launch counts
            if np_ and d < t <= 1 << 20 and np_ <= MAX_ITEMS and s <= 1 << 20:
                assert rc == abi.RT_ERR_UNSUPPORTED and np_ * -(-(t - d) // max(s, 1)) > MAX_ITEMS // 2, case
            continue
        ok += 1
        assert n_items == np_ * nsub <= MAX_ITEMS, case
        assert base == (d - d % 128 if S % 128 == 0 else d), case
        # first and last item from the formula of rt_progressive_plan.hpp
        assert max(d, base) == d and base + nsub * S >= t > base + (nsub - 1) * S, case
        assert base + S > d, case                         # the first item is not empty
        if s:
            assert S == s, case
        elif nsub > 1:
            split += 1
            assert S % 128 == 0, case
        else:
            assert S == t - d and base == d, case         # one item per pixel: the window itself
    assert ok > len(cases) // 2 and split > 50
