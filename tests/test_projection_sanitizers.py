"""AddressSanitizer + UndefinedBehaviorSanitizer build of the host ray generators (csrc/rt_projection.hpp, pure host
C++: what rt_camera_rays runs), in the style of tests/test_sanitizers.py: a stand-alone program
(tests/sanitize/projection_san.cpp) built with g++ `-fsanitize=address,undefined -fno-sanitize-recover=all`, so any
report aborts it with a non-zero status.  It allocates every array at its exact size, runs each model in both
precisions over odd and even frames and grids, the refusals, and sizes past the limits; its return codes, ray counts,
zero-direction counts and checksums must equal what the library gives through rt.projections.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import rt_mi355x as rt
from rt_mi355x import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

FROM, AT, UP = (13.0, 2.0, 3.0), (0.5, 0.25, -0.125), (0.0, 1.0, 0.0)


@pytest.fixture(scope="module")
def projection_san(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("san") / "projection_san")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-o", out,
                    os.path.join(REPO, "tests", "sanitize", "projection_san.cpp")], check=True)
    return out


def _cases():
    ok, refused = [], []
    for model in (0, 1, 2):
        for f32 in (0, 1):
            for w, h, grid in ((1, 1, 1), (9, 5, 1), (4, 6, 3), (7, 7, 2), (33, 2, 5)):
                ok.append((model, w, h, grid, f32, FROM, AT, UP, 200.0, 6.0))
    ok.append((2, 8, 8, 2, 0, FROM, AT, UP, 360.0, 1.0))
    ok.append((0, 5, 3, 1, 1, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (1.0, 1.0, 0.0), 0.0, 1e-3))   # angle unused by ortho
    for kw in (dict(w=0), dict(h=0), dict(grid=0), dict(model=3), dict(at=FROM),
               dict(frm=(0.0, 0.0, 0.0), at=(0.0, 0.0, -2.0), up=(0.0, 0.0, 3.0)),   # up along the view axis
               dict(at=(float("nan"), 0.0, 0.0)), dict(up=(0.0, float("inf"), 0.0)), dict(model=2, angle=0.0),
               dict(model=2, angle=360.5), dict(model=2, angle=float("nan")), dict(model=0, extent=0.0),
               dict(model=0, extent=-1.0), dict(model=0, extent=float("inf"))):
        c = dict(model=1, w=4, h=4, grid=1, f32=0, frm=FROM, at=AT, up=UP, angle=180.0, extent=1.0)
        c.update(kw)
        refused.append((c["model"], c["w"], c["h"], c["grid"], c["f32"], c["frm"], c["at"], c["up"], c["angle"], c["extent"]))
    refused.append((1, 0x10000, 0x8000, 1, 0, FROM, AT, UP, 180.0, 1.0))   # 2^31 pixels
    refused.append((1, 4, 4, 1025, 1, FROM, AT, UP, 180.0, 1.0))
    return ok, refused


def _text(c):
    model, w, h, grid, f32, frm, at, up, angle, extent = c
    return " ".join([str(model), str(w), str(h), str(grid), str(f32)] + [repr(float(v)) for v in (*frm, *at, *up, angle, extent)])


def test_ray_generators_under_asan_ubsan(projection_san, lib):
    ok, refused = _cases()
    r = subprocess.run([projection_san], input="\n".join(_text(c) for c in ok + refused), capture_output=True, text=True,
                       env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(ok) + len(refused)
    zeros = 0
    for c, line in zip(ok, lines):
        model, w, h, grid, f32, frm, at, up, angle, extent = c
        rc, n, zero, csum = line.split()
        o, d = rt.projections.camera_rays(model, w, h, frm, at, up, grid=grid, precision="f32" if f32 else "f64",
                                          angle_deg=angle, extent=extent, lib=lib)
        assert int(rc) == abi.RT_OK and int(n) == w * h * grid * grid == d.shape[0] * d.shape[1], c
        assert int(zero) == int((d == 0).all(-1).sum()), c
        # the same values in the same order: the sum over rays of (o + d) components, accumulated in double
        want = 0.0
        for oo, dd in zip(o.reshape(-1, 3).astype(np.float64), d.reshape(-1, 3).astype(np.float64)):
            for a in range(3):
                want += oo[a] + dd[a]
        assert float.fromhex(csum) == want, c
        zeros += int(zero)
    assert zeros > 0, "some fisheye case has pixels outside the image circle"
    for c, line in zip(refused, lines[len(ok):]):
        rc, n, zero, _ = line.split()
        big = c[1] * c[2] > 0x7FFFFFFF or c[3] > 1024
        assert int(rc) == (abi.RT_ERR_UNSUPPORTED if big else abi.RT_ERR_INVALID) and int(n) == 0, c
