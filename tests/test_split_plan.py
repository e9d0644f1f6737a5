"""The sample-parallel path's plan (csrc/rt_split_plan.hpp, rt_split_plan in the C ABI) and its kernel_id
bit, on the CPU: no GPU here.

The plan deals a pixel's samples to work items of S samples; the grid below is checked through the library
(ctypes) and through a stand-alone AddressSanitizer + UBSan program (tests/sanitize/split_plan_san.cpp) that
includes the same header."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

from rt_mi355x import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355x.h")

PIXELS = [1, 12, 144, 2304, 6144, 10 ** 6]
SPPS = [1, 64, 100, 512, 4096, 70001, 1 << 20]
WAVES = [4096, 5120, 6144]
GRID = list(itertools.product(PIXELS, SPPS, WAVES))
MAX_ITEMS = 0x7FFFFFFF


def plan(lib, n_pixels, spp, waves):
    s, n = ctypes.c_uint32(0xDEAD), ctypes.c_uint64(0xDEAD)
    rc = lib.rt_split_plan(n_pixels, spp, waves, ctypes.byref(s), ctypes.byref(n))
    return rc, s.value, n.value


def check_plan(n_pixels, spp, waves, rc, S, n_items):
    """The properties every plan of the grid must have."""
    key = (n_pixels, spp, waves)
    if rc != abi.RT_OK:
        # the only refusal inside the ABI's limits: more items than a launch can count
        assert rc == abi.RT_ERR_UNSUPPORTED, key
        return
    assert 1 <= S <= spp, key
    nsub = -(-spp // S)
    assert n_items == n_pixels * nsub and n_items <= MAX_ITEMS, key
    if nsub == 1:
        assert S == spp, key                      # the one-item case
    else:
        assert S % 128 == 0 and S >= 128, key
    # item j holds [j S, min(spp, (j + 1) S)): [0, spp) exactly once and no empty item, which is
    # (nsub - 1) S < spp <= nsub S; enumerated as well where a pixel has few items
    assert (nsub - 1) * S < spp <= nsub * S, key
    if nsub <= 8192:
        covered = 0
        for j in range(nsub):
            b, e = j * S, min(spp, (j + 1) * S)
            assert b == covered and e > b, key
            covered = e
        assert covered == spp, key
    if n_pixels >= 8 * waves:
        assert nsub == 1, key
    if n_pixels < waves and spp >= 256:
        assert nsub > 1, key


def test_plan_grid(lib):
    split = 0
    for n_pixels, spp, waves in GRID:
        rc, S, n_items = plan(lib, n_pixels, spp, waves)
        check_plan(n_pixels, spp, waves, rc, S, n_items)
        split += rc == abi.RT_OK and n_items > n_pixels
    assert split > len(GRID) // 4   # the grid is not all one-item plans


def test_plan_aims_at_the_resident_waves(lib):
    """About 8 items per resident wave where the samples allow it: between 4 and 9 per wave once each item
    can be a whole number of 128-sample grains (one pixel at 2^20 spp has 8 192 grains, so no more items)."""
    for n_pixels, waves in ((12, 5120), (144, 5120), (2304, 4096)):
        rc, S, n_items = plan(lib, n_pixels, 1 << 20, waves)
        assert rc == abi.RT_OK and 4 * waves <= n_items <= 9 * waves + n_pixels, (n_pixels, waves, S, n_items)
    assert plan(lib, 1, 1 << 20, 5120) == (abi.RT_OK, 128, 8192)


def test_plan_edges(lib):
    assert plan(lib, 0, 16, 5120) == (abi.RT_ERR_INVALID, 0, 0)
    assert plan(lib, 16, 0, 5120) == (abi.RT_ERR_INVALID, 0, 0)
    assert plan(lib, 16, 512, 0) == (abi.RT_OK, 512, 16)            # no waves: one item per pixel
    assert plan(lib, 16, (1 << 20) + 1, 5120)[0] == abi.RT_ERR_UNSUPPORTED
    assert plan(lib, 1 << 31, 16, 5120)[0] == abi.RT_ERR_UNSUPPORTED
    assert plan(lib, MAX_ITEMS, 16, 5120) == (abi.RT_OK, 16, MAX_ITEMS)
    n = ctypes.c_uint64()
    assert lib.rt_split_plan(1, 1, 1, None, ctypes.byref(n)) == abi.RT_ERR_INVALID
    assert b"rt_split_plan" in lib.rt_last_error()


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_plan_under_asan_ubsan(lib, tmp_path):
    """The header alone, in a stand-alone program built with ASan + UBSan: the grid plus the edge values; its
    plans equal the library's."""
    exe = str(tmp_path / "split_plan_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-o", exe, os.path.join(REPO, "tests", "sanitize", "split_plan_san.cpp")],
                   check=True)
    cases = GRID + [(0, 16, 5120), (16, 0, 5120), (16, 512, 0), (0, 0, 0), (1, 1, 0xFFFFFFFF), (MAX_ITEMS, 1 << 20, 0xFFFFFFFF),
                    (1 << 31, 1, 1), (1, (1 << 20) + 1, 1), (MAX_ITEMS, 300, 0xFFFFFFFF), (2 ** 64 - 1, 1 << 20, 0xFFFFFFFF)]
    text = "\n".join(f"{a} {b} {c}" for a, b, c in cases) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for (n_pixels, spp, waves), line in zip(cases, lines):
        got = tuple(int(x) for x in line.split())
        assert got == plan(lib, n_pixels, spp, waves), (n_pixels, spp, waves)
        if (n_pixels, spp, waves) in GRID:
            check_plan(n_pixels, spp, waves, *got)


def test_kernel_split_bit_mirrors_the_header(tmp_path):
    """RT_KERNEL_SPLIT in the header and in abi.py decode alike; ids without the bit print as before."""
    ids = [0x808C, 0x81F9, 0x808C | 0x200, 0x828A, 0x8389, 0]
    src = tmp_path / "split_bit.c"
    src.write_text('#include <stdio.h>\n#include "rt_mi355x.h"\nint main(void) {\n' +
                   "".join(f'  printf("%u\\n", RT_KERNEL_SPLIT({i:#x}u));\n' for i in ids) + "  return 0;\n}\n")
    exe = tmp_path / "split_bit"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [abi.RT_KERNEL_SPLIT(i) for i in ids] == [0, 0, 1, 1, 1, 0]
    assert re.search(r"#define\s+RT_KERNEL_SPLIT\(id\)\s+\(\(\(id\)\s*>>\s*9\)\s*&\s*1u\)", open(HEADER).read())
    # the two names tests/test_abi.py pins
    assert abi.kernel_name(0x808C) == "trace_paths<float,6,false,0,true,false>"
    assert abi.kernel_name(0x81F9) == "trace_paths<double,4,true,3,true,true>"
    assert abi.kernel_info(0x808C)["split"] is False and abi.kernel_info(0) is None
    # fp32 W5 pinhole split kernel; fp64 W4 pinhole mega split kernel
    assert abi.kernel_name(0x828A) == "trace_paths_split<float,5,true,false>"
    assert abi.kernel_name(0x8389) == "trace_paths_split<double,4,true,true>"
    k = abi.kernel_info(0x8389)
    assert k["split"] and k["T"] == "double" and k["W"] == 4 and k["camq"] and k["mega"] and not k["root2"] and k["mode"] == 0


def test_entry_points_are_exported(lib):
    assert {"rt_render_split_async", "rt_split_plan"} <= set(abi.EXPORTED)
    for name in ("rt_render_split_async", "rt_split_plan"):
        assert hasattr(lib, name)
    assert os.path.join(abi.PKG_DIR, "csrc", "rt_split_plan.hpp") in abi.SOURCE_FILES


def test_renderer_rejects_a_bad_samples_per_item():
    """GpuRenderer.render_flat's samples_per_item is None, 0 or a positive count (checked before any GPU call)."""
    from rt_mi355x.renderer import split_argument
    assert split_argument(None) is None and split_argument(0) == 0 and split_argument(128) == 128
    for bad in (-1, 1.5, "auto", True):
        with pytest.raises((ValueError, TypeError)):
            split_argument(bad)
