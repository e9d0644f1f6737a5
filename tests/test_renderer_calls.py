"""The C calls rt_mi355x.renderer makes, replayed over a recording stand-in for the library (no GPU, no built
library): every public method's calls, in order, with their arguments, against tests/golden/renderer_calls.json
(written by tests/golden/make_renderer_golden.py), and what each method frees when one of its calls fails."""
import json
import os

import pytest

import renderer_recording as rec
from rt_mi355x import abi, RtError

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "renderer_calls.json")))


def test_every_case_is_recorded():
    assert list(GOLDEN) == list(rec.CALL_CASES)


@pytest.mark.parametrize("name", list(rec.CALL_CASES))
def test_calls_replay_exactly(name):
    fake, got = rec.run_case(rec.CALL_CASES[name])
    got = json.loads(json.dumps(got))   # tuples and lists alike, as the file has them
    want = GOLDEN[name]
    for k, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"call {k}"
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    assert got["result"] == want["result"]
    assert sorted(fake.freed) == sorted(fake.handed), "a device buffer was not freed exactly once"


def test_what_the_recorded_cases_pin():
    """The golden file holds the properties the cases were chosen for (so a regenerated file cannot lose them)."""
    names = lambda case: [c[0] for c in GOLDEN[case]["calls"]]
    # a device round trip frees in allocation order
    for case in ("render_flat_linear", "guides_flat", "query_per_ray", "render_rays_per_ray_linear"):
        calls = GOLDEN[case]["calls"]
        freed = [c[2]["dev"] for c in calls if c[0] == "rt_device_free"]
        assert freed == list(range(names(case).count("rt_device_alloc"))) and len(freed) >= 2, case
    # allocation follows `want`, the call's arguments GUIDE_NAMES: (albedo, normal, depth, coverage) = (1, NULL, 0, NULL)
    call = [c for c in GOLDEN["guides_flat_depth_albedo"]["calls"] if c[0] == "rt_render_guides_async"][0]
    assert call[7:11] == [{"dev": 1}, None, {"dev": 0}, None]
    # n == 0: the scene is set, nothing else is called
    assert names("query_empty") == names("render_rays_empty") == ["rt_context_create", "rt_context_set_scene"]
    # the same FlatScene is uploaded once; a failed upload leaves no scene
    assert names("second_render").count("rt_context_set_scene") == 2 and GOLDEN["second_render"]["result"] == [False, True]
    assert GOLDEN["failed_upload"]["result"][2] is True
    # the session refreshes its counts between the launch and the collect
    session = names("session")
    i = session.index("rt_progressive_extend_async")
    assert session[i + 1:i + 3] == ["rt_progressive_counts", "rt_context_collect"]
    # RT_ERR_RANGE: render and adaptive raise, render_flat and a session hand the code on, progressive flags the step
    text = "rt_mi355x error 3: a pixel channel exceeded 2.0 (reference: Color::to_u8_array panics)"
    for case in ("render_range", "adaptive_range"):
        assert GOLDEN[case]["result"] == {"raises": "RtError", "text": text}
    assert GOLDEN["render_flat_range"]["result"][3] == GOLDEN["render_rays_range"]["result"][3] == abi.RT_ERR_RANGE
    assert all(step[2]["RenderStat"][4] is True for step in GOLDEN["progressive_range"]["result"])
    # a closed session refuses the calls that need it, and rt_context_destroy ends an open one without rt_progressive_end
    assert GOLDEN["session"]["result"].count("the progressive session is closed") == 5
    assert names("close_with_session")[-1] == "rt_context_destroy" and "rt_progressive_end" not in names("close_with_session")


def sweep():
    for name, setup in rec.FAILURE_CASES.items():
        fake = rec.FakeLib()
        call = setup(fake)
        base = len(fake.calls)
        call()
        for k, c in enumerate(fake.calls[base:]):
            if c[0] != "rt_device_free":   # its return value is not looked at: nothing to do about a failed free
                yield pytest.param(name, k, id=f"{name}-{k}-{c[0]}")


@pytest.mark.parametrize("name,k", list(sweep()))
def test_no_leak_when_a_call_fails(name, k):
    fake = rec.FakeLib()
    call = rec.FAILURE_CASES[name](fake)
    fake.fail_at = len(fake.calls) + k
    with pytest.raises(RtError) as e:
        call()
    assert e.value.code == abi.RT_ERR_HIP and "injected failure" in str(e.value)
    assert sorted(fake.freed) == sorted(fake.handed)   # each pointer handed out, freed exactly once
    assert fake.freed == sorted(fake.freed)            # and in allocation order
