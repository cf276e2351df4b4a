#!/usr/bin/env python3
"""Golden record of the attention dispatch: what ``ir_shared_attn_kernel_name`` (and, for a refused call,
``ir_last_error_string``) answers over the grid of dispatch_grid.py.  Recorded ONCE, from the library built at the commit before
the dispatch decision became one function (two restatements of it existed then: the launch's and the name's), so that the single
decision is held to what shipped:

    git worktree add <dir> <that commit> && IR_OUT=<dir>/lib.so bash <dir>/instantrestore_amd/csrc/build.sh
    IR_LIB_PATH=<dir>/lib.so python -B tests/golden/make_golden_dispatch.py

The fixture holds every distinct (name, error) pair once and the grid as indices into that list, one row per IR_ATTN_W128
setting (unset, 0, 1)."""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dispatch_grid as DG  # noqa: E402

OUT = os.path.join(HERE, "dispatch_golden.npz")


def main():
    runs = DG.record_in_children(os.environ.get("IR_LIB_PATH"))
    table = sorted({tuple(e) for run in runs for e in run})
    index = {e: i for i, e in enumerate(table)}
    assert len(table) < 256
    idx = np.array([[index[tuple(e)] for e in run] for run in runs], dtype=np.uint8)
    np.savez_compressed(OUT, index=idx, table=np.frombuffer(json.dumps(table).encode(), dtype=np.uint8))
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", idx.shape, "entries,", len(table), "distinct answers")


if __name__ == "__main__":
    main()
