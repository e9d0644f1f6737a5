"""bench.py's host logic on the CPU: the N-rank self-launch, the world-size check, and the PMC
staleness rule (no GPU work: --probe-dist stops after the process group is up)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(RT_BENCH_BACKEND="gloo", **kw)
    return env


def test_gpus_2_without_a_launcher_runs_two_ranks():
    """`python bench.py --gpus 2` (as the driver runs it) starts 2 ranks itself: n_gpus 2, world 2."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--probe-dist"], capture_output=True, text=True,
                       env=_env(), timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["dist"]["world_size_initialised"] == 2
    assert line["dist"]["ranks"] == [0, 1]


def test_world_size_mismatch_exits_nonzero():
    """A rank whose world is not --gpus refuses to report (no silent 1-GPU line labelled N GPUs)."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--probe-dist"], capture_output=True, text=True,
                       env=_env(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                                MASTER_PORT="29517"), timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_full_is_off_by_default(monkeypatch):
    """A plain run times the headline leg only; the other precision and the CPU baseline need --full."""
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "d" and a.other_precision == 1 and a.cpu_seconds > 0


def test_dump_outputs_whole_frame_and_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs: a frame within the size limit is written whole as float32; a larger one as a fixed
    pixel sample with its indices, the same from call to call and under the limit."""
    b = _bench_module()
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    b.dump_outputs(str(tmp_path / "a"), img)
    got = np.load(tmp_path / "a" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)
    assert os.listdir(tmp_path / "a") == ["image.npy"]
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 9 * 7 * 3 * 4 - 1)   # one byte too small for the frame
    monkeypatch.setattr(b, "DUMP_SAMPLE_PIXELS", 10)
    for d in ("b", "c"):
        b.dump_outputs(str(tmp_path / d), img)
    s, i = np.load(tmp_path / "b" / "image.npy"), np.load(tmp_path / "b" / "image_index.npy")
    assert s.dtype == np.float32 and s.shape == (10, 3) and i.dtype == np.float64 and i.shape == (10,)
    assert len(set(i.tolist())) == 10 and np.array_equal(s, img.reshape(-1, 3)[i.astype(np.int64)])
    assert np.array_equal(s, np.load(tmp_path / "c" / "image.npy")) and np.array_equal(i, np.load(tmp_path / "c" / "image_index.npy"))
    assert b.DUMP_SAMPLE_PIXELS * (3 * 4 + 8) <= b.DUMP_MAX_BYTES


def _run_bench(*argv):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", *argv], capture_output=True, text=True,
                       env={k: v for k, v in _env().items() if k != "RT_BENCH_BACKEND"}, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_one_leg_and_dumps_its_frame(tmp_path):
    """A plain run on config A (fp32): exactly --steps timed steps, no other-precision leg, no CPU baseline;
    --dump-outputs writes the frame of the last timed step, which equals the oracle's fp32 golden frame."""
    out = tmp_path / "dump"
    line = _run_bench("--config", "A", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["unit"] == "Msamples/s"
    assert "f64" not in line and "f32" not in line and line["cpu_baseline"] is None
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
    # value and ms_per_step are the same measurement, each rounded to 3 decimals (0.0005 ms on the latter)
    assert line["value"] == pytest.approx(400 * 225 * 16 / (line["ms_per_step"] * 1e-3) / 1e6,
                                          rel=0.0006 / line["ms_per_step"] + 1e-4)
    assert line["dist"]["per_rank"][0]["pixels"] == 400 * 225
    want = np.load(os.path.join(REPO, "tests", "golden", "config_a_f32.npz"))
    assert int(want["seed"]) == 0x5EED0001 and (int(want["spp"]), int(want["max_bounces"])) == (16, 8)
    got = np.load(out / "image.npy")
    assert got.dtype == np.float32 and os.listdir(out) == ["image.npy"]
    np.testing.assert_array_equal(got, want["rgb8"])


@pytest.mark.gpu
def test_full_run_adds_the_other_precision(tmp_path):
    """--full on config A (fp64 headline): the fp32 leg is timed after it under the line's "f32" key, and
    the dumped frame is still the headline leg's (the oracle's fp64 golden frame)."""
    out = tmp_path / "dump"
    line = _run_bench("--config", "A", "--precision", "f64", "--steps", "2", "--warmup", "1", "--full",
                      "--cpu-seconds", "0", "--dump-outputs", str(out))
    assert line["dtype"] == "f64" and line["f32"]["value"] > 0 and line["f32"]["ms_per_step"] > 0
    assert "f64" not in line and line["cpu_baseline"] is None
    want = np.load(os.path.join(REPO, "tests", "golden", "config_a.npz"))
    np.testing.assert_array_equal(np.load(out / "image.npy"), want["rgb8"])


def test_pmc_record_from_other_sources_is_stale():
    b = _bench_module()
    rec = {"hbm_bytes_per_launch": 4.7e10, "valu_busy": 0.63, "commit": "656c11f74452", "src_hash": "aaaaaaaaaaaa",
           "launch_ms": 39.5, "issue_frac": 0.91, "issue_frac_vs_ubench": 1.01, "pmc_flop_frac": 0.27}
    f = b.pmc_fields(rec, "bbbbbbbbbbbb", "profiles/pmc.json")
    assert f["pmc_source"]["stale"] is True and f["traffic"] is None and f["valu_busy"] is None
    assert f["issue_frac"] is None and f["pmc_flop_frac"] is None
    f = b.pmc_fields(rec, "aaaaaaaaaaaa", "profiles/pmc.json")
    assert f["pmc_source"]["stale"] is False and f["traffic"] == 4.7e10 and f["valu_busy"] == 0.63
    assert f["issue_frac"] == 0.91 and f["issue_frac_vs_ubench"] == 1.01 and f["pmc_flop_frac"] == 0.27
    old = dict(rec)
    del old["src_hash"]   # a record written before the hash existed
    assert b.pmc_fields(old, "aaaaaaaaaaaa", "x")["pmc_source"]["stale"] is True
    assert b.pmc_fields({}, "aaaaaaaaaaaa", "x") == {"traffic": None, "valu_busy": None, "issue_frac": None,
                                                     "issue_frac_vs_ubench": None, "pmc_flop_frac": None,
                                                     "pmc_source": None}
