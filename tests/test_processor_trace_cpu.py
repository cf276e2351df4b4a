"""``SharedAttnProcessor.forward`` makes the calls it made before: every case of ``tests/processor_trace.py`` against the traces in
``tests/golden/processor_trace.json``, which were recorded from the commit named in the fixture's header.

A case that succeeds must leave the same calls with the same arguments, the same output and the same result attributes.  A case
that is refused must raise the same exception with the same text, and whatever it launched before raising must be a prefix of
what the recorded call launched (a refusal may come earlier, never after different work)."""
import json
import os

import pytest

import processor_trace

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "processor_trace.json")) as _f:
    GOLDEN = json.load(_f)
NAMES = list(processor_trace.cases())


def test_fixture_and_case_list_agree():
    assert GOLDEN["header"]["commit"]
    assert sorted(GOLDEN["cases"]) == sorted(NAMES)
    ends = [c["end"] for c in GOLDEN["cases"].values()]
    assert sum(e == "ok" for e in ends) >= 60 and sum(e != "ok" for e in ends) >= 40
    for name, c in GOLDEN["cases"].items():
        assert (c["end"] != "ok") == name.startswith("refused_"), name


@pytest.mark.parametrize("name", NAMES)
def test_trace(name):
    import instantrestore_amd.attn_processors as ap
    want = GOLDEN["cases"][name]
    got = json.loads(json.dumps(processor_trace.run_case(ap, processor_trace.cases()[name])))
    assert got["end"] == want["end"]
    if want["end"] == "ok":
        assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
        assert got == want
    else:
        assert got["calls"] == want["calls"][:len(got["calls"])]
