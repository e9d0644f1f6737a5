"""Every exception rt_mi355x.renderer's argument checks raise, by type and full text, against
tests/golden/renderer_messages.json (written by tests/golden/make_renderer_golden.py).  No GPU, no built library:
the renderers here have no library at all, so a check that came after the first use of it would not get to raise."""
import json
import os

import pytest

import renderer_recording as rec

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "renderer_messages.json")))


def test_every_case_is_recorded():
    assert list(GOLDEN) == list(rec.MESSAGE_CASES)


@pytest.mark.parametrize("name", list(rec.MESSAGE_CASES))
def test_message(name):
    kind, text, where = rec.run_message(rec.MESSAGE_CASES[name])
    assert [kind, text] == GOLDEN[name]
    assert where is not None, "raised outside the Python layer's own checks"


def test_the_cases_reach_every_raise_of_the_argument_checks():
    """What is left out is covered by test_renderer_calls.py: the RT_ERR_RANGE raises and the closed session."""
    unreached = rec.unreached_raises()
    assert [t for t in unreached if not rec.allowed_unreached(t)] == []
    assert len(rec.raise_statements()) > len(unreached)
