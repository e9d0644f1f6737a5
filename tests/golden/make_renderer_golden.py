#!/usr/bin/env python3
"""Records what rt_mi355x.renderer does over the recording stand-in for the library (tests/renderer_recording.py):

  tests/golden/renderer_calls.json      per case, the C calls in order with their arguments, and what came back
  tests/golden/renderer_messages.json   per case, the exception an argument check raises: type and full text

  python tests/golden/make_renderer_golden.py

Neither needs the built library or a GPU.  tests/test_renderer_calls.py and tests/test_renderer_messages.py replay
the same cases and compare exactly, so a change of the Python layer that is meant to keep its behaviour leaves both
files as they are.  The raise statements of the checked sources that no message case reaches are printed; they may
only be the ones test_renderer_calls.py covers (allowed_unreached).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "rust-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import renderer_recording as rec  # noqa: E402


def dump_calls(records):
    """One call per line: the file stays readable and a changed call shows as one changed line."""
    out = ["{"]
    for i, (name, r) in enumerate(records.items()):
        out.append(f' {json.dumps(name)}: {{"calls": [')
        out += [f'  {json.dumps(c)}{"," if k + 1 < len(r["calls"]) else ""}' for k, c in enumerate(r["calls"])]
        out.append(f' ], "result": {json.dumps(r["result"])}}}{"," if i + 1 < len(records) else ""}')
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    calls = {name: rec.run_case(case)[1] for name, case in rec.CALL_CASES.items()}
    with open(os.path.join(HERE, "renderer_calls.json"), "w") as f:
        f.write(dump_calls(calls))
    messages = {}
    for name, call in rec.MESSAGE_CASES.items():
        kind, text, where = rec.run_message(call)
        assert where is not None, f"{name}: raised outside {rec.CHECKED_SOURCES}: {kind}: {text}"
        messages[name] = [kind, text]
    with open(os.path.join(HERE, "renderer_messages.json"), "w") as f:
        json.dump(messages, f, indent=0)
        f.write("\n")
    unreached = rec.unreached_raises()
    print(f"{len(calls)} call cases, {len(messages)} message cases; raise statements of {rec.CHECKED_SOURCES} not reached:")
    for text in unreached:
        print("   ", " ".join(text.split()))
    stray = [t for t in unreached if not rec.allowed_unreached(t)]
    assert not stray, stray


if __name__ == "__main__":
    main()
