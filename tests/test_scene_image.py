"""The scene image (csrc/rt_layout.hpp: build_scene_image, every device table of a scene, built on the host)
under AddressSanitizer + UBSan, without a GPU: tests/sanitize/layout_san.cpp is plain C++ (rt_layout.hpp needs
no HIP), built with the flags of tests/test_sanitizers.py.  It builds the image of each scene below and checks
the image's invariants itself (every scene index once in ridx, every table's length against the counts, the
local levels present exactly with a mega level, n_gg only up to 16 mega groups, clusters of at most 16).

Scenes: rt.scenes.random_spheres(n) at the counts of test_layout_padding_shapes and test_mega_walk_shapes
(the smallest at which each branch of the layout is reached) plus 16500, the first of them with more than 16
mega groups, and every scene of tests/edge_scenes.py (ties, signed and zero radii, the 1e19 and 1e25 scales).
"""
import os
import subprocess

import pytest

import rt_mi355x as rt
import edge_scenes as es
from test_sanitizers import ENV, SAN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 1, 17, 20, 261, 1029, 2053, 2600, 3000, 4100, 16500, 70000]


@pytest.fixture(scope="module")
def layout_san(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("san") / "layout_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-o", out,
                    os.path.join(REPO, "tests", "sanitize", "layout_san.cpp")], check=True)
    return out


def _scene_text(name, flat):
    t = [name, str(flat.n_spheres), str(len(flat.materials))]
    for c, r, m in zip(flat.center.tolist(), flat.radius.tolist(), flat.material.tolist()):
        t.append(f"{c[0]!r} {c[1]!r} {c[2]!r} {r!r} {int(m)}")
    for m in flat.materials:
        a = m.to_abi()
        t.append(f"{a.kind} {a.hollow} {a.albedo[0]!r} {a.albedo[1]!r} {a.albedo[2]!r} {a.fuzz!r} {a.ior!r}")
    return "\n".join(t)


def _random(n):
    """rt.scenes.random_spheres(n); below its minimum of 4 spheres, the first n of random_spheres(4)."""
    flat = rt.scenes.random_spheres(max(n, 4)).flatten()
    if n < 4:
        flat = rt.FlatScene(flat.center[:n], flat.radius[:n], flat.material[:n], flat.materials)
    assert flat.n_spheres == n
    return flat


def _scenes():
    out = [(f"random{n}", _random(n)) for n in COUNTS]
    edge = {
        "twins": es.twins(), "twins_swap": es.twins(swap=True), "twins_mega": es.twins_mega(),
        "stack": es.stack(), "stack_reverse": es.stack(reverse=True),
        "radii": es.radii(), "radii_abs": es.radii(absolute=True), "materials": es.materials(),
        "scaled_empty": es.scaled(1e6, empty=True),
    }
    edge.update({f"scaled_{s:g}": es.scaled(s) for s in es.SCALES})
    edge.update({f"needle_{k}": es.needle(k) for k in es.NEEDLES})
    edge.update({name: build() for name, build in es.LAYOUT_FAMILIES.items()})
    return out + [(name, flat) for name, (flat, _cam) in edge.items()]


def test_scene_image_under_asan_ubsan(layout_san):
    scenes = _scenes()
    text = "\n".join(_scene_text(name, flat) for name, flat in scenes) + "\n"
    r = subprocess.run([layout_san], input=text, capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    rows = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.strip().split("\n")}
    assert list(rows) == [name for name, _ in scenes]
    for name, flat in scenes:
        assert rows[name][0] == flat.n_spheres
    # the scenes reach every branch of the layout: up to 32 top groups (no mega level, no super records in the
    # camera cull) and more; the giga pre-test on and, past 16 mega groups, off; always-exact spheres and none
    col = lambda k: {name: v[k] for name, v in rows.items()}   # noqa: E731
    n_xg, n_top, n_mg, n_gg, n_supc = col(1), col(3), col(4), col(5), col(6)
    assert n_top["random1029"] <= 32 and n_mg["random1029"] == 0 and n_supc["random1029"] == 0
    assert n_top["random2053"] > 32 and n_mg["random2053"] > 0 and n_supc["random2053"] > 0 and n_mg["twins_mega"] > 0
    assert n_gg["random4100"] > 0 and n_mg["random16500"] == 17 and n_gg["random16500"] == 0 and n_gg["random70000"] == 0
    assert n_xg["uniform"] == 0 and n_xg["random261"] > 0
