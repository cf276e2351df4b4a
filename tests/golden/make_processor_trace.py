"""Writes ``processor_trace.json``: what every case of ``tests/processor_trace.py`` leaves behind - recorded results only.

    python tests/golden/make_processor_trace.py --repo <checkout> --commit <its commit>

``--repo``: the checkout whose ``instantrestore_amd`` is traced (default: this one).  The fixture is recorded from the commit
BEFORE a change of the processors and then held by ``tests/test_processor_trace_cpu.py`` after it; ``--commit`` goes into the
header."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repo", default=os.path.dirname(os.path.dirname(HERE)))
    p.add_argument("--commit", required=True)
    p.add_argument("--out", default=os.path.join(HERE, "processor_trace.json"))
    a = p.parse_args()
    sys.path[:0] = [os.path.abspath(a.repo), os.path.dirname(HERE)]
    import processor_trace
    import instantrestore_amd.attn_processors as ap
    assert os.path.abspath(ap.__file__).startswith(os.path.abspath(a.repo) + os.sep), ap.__file__
    doc = {"header": {"commit": a.commit, "module": "instantrestore_amd/attn_processors.py", "cases": "tests/processor_trace.py",
                      "written_by": "tests/golden/make_processor_trace.py"},
           "cases": processor_trace.run_all(ap)}
    with open(a.out, "w") as f:
        f.write("{\n\"header\": " + json.dumps(doc["header"]) + ",\n\"cases\": {\n")
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc["cases"].items()))
        f.write("\n}}\n")
    print(f"{len(doc['cases'])} cases -> {a.out}")


if __name__ == "__main__":
    main()
