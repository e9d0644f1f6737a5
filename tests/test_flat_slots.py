"""The flat slot table (csrc/rt_layout.hpp, pack_flat), the records nearest_hit's per-lane exact tests gather from,
under AddressSanitizer + UBSan, without a GPU: tests/sanitize/flat_slots_san.cpp is plain C++ with its own main,
built with the flags of tests/test_sanitizers.py and run directly.  For 1, 16, 17, 500 and 2048 filtered
spheres, with and without always-exact and big spheres, it checks every slot's record bit for bit against the
centre and r^2 of the slot's cluster block in the fp32 filter stream and the block's index word against ridx,
dummies included; a violation exits non-zero.

The second test pins the structure of the scenes of tests/test_gpu_sweep_flush.py (supers, always-exact spheres,
no mega level) with tests/sanitize/layout_san.cpp, so those GPU cases keep reaching what they are aimed at.
"""
import os
import subprocess

import pytest

from test_sanitizers import ENV, SAN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 16, 17, 500, 2048]


@pytest.fixture(scope="module")
def flat_slots_san(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("san") / "flat_slots_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-o", out,
                    os.path.join(REPO, "tests", "sanitize", "flat_slots_san.cpp")], check=True)
    return out


def test_flat_slots_under_asan_ubsan(flat_slots_san):
    r = subprocess.run([flat_slots_san], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    assert list(rows) == [f"slab{n}{tag}" for n in COUNTS for tag in ("", "_exact")]
    for n in COUNTS:
        ns, n_xg, n_xs, n_top, n_mg, slots, dummies = rows[f"slab{n}"]
        assert ns == n and n_xs == 0 and n_xg == 0 and n_mg == 0
        assert slots == 64 * n_top + 64 and dummies == slots - n
        assert n_top == max(1, -(-n // 64))          # whole supers of 64 slots
        ns, n_xg, n_xs, n_top_x, n_mg, slots, dummies = rows[f"slab{n}_exact"]
        assert ns == n + 4 and n_mg == 0 and dummies == slots - ns
        if n >= 16:   # the ground and the three radius-1 spheres join the always-exact group, the rest stay filtered
            assert n_xs == 4 and n_xg == 1 and n_top_x == n_top
    # 2048 filtered spheres fill the 32 supers of the largest scene without a mega level
    assert rows["slab2048"][3] == 32 and rows["slab2048_exact"][3] == 32


@pytest.fixture(scope="module")
def layout_san(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("san") / "layout_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-o", out,
                    os.path.join(REPO, "tests", "sanitize", "layout_san.cpp")], check=True)
    return out


def test_gpu_flush_scenes_have_their_structure(layout_san):
    """The scenes of tests/test_gpu_sweep_flush.py through build_scene_image (tests/sanitize/layout_san.cpp, which
    checks the image's invariants): each has the supers, always-exact spheres and (no) mega level its case is
    about (STRUCTURE), so a drift of build_layout's rules (the 8x median rule, kBigRatio, the k-d alignment) shows
    here and not as a GPU test that still passes beside the path it was aimed at."""
    import test_gpu_sweep_flush as gf
    from test_scene_image import _scene_text
    assert set(gf.STRUCTURE) == set(gf.CASES)
    flats = {name: case[1]()[0] for name, case in gf.CASES.items()}
    text = "\n".join(_scene_text(name, flat) for name, flat in flats.items()) + "\n"
    r = subprocess.run([layout_san], input=text, capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    # layout_san's line: name n n_xg n_xs n_top n_mg n_gg n_supc
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    got = {name: (v[3], v[2], v[4]) for name, v in rows.items()}
    assert got == gf.STRUCTURE
    for name, flat in flats.items():
        n, n_xg, n_xs = rows[name][0], rows[name][1], rows[name][2]
        assert n == flat.n_spheres and n_xs == 1 and n_xg == 1   # the ground alone is always exact: no shell or big sphere
