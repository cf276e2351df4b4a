"""The attention dispatch against its golden record (tests/golden/dispatch_golden.npz, recorded from the library of the commit
before ``ir_attn_choose`` existed: make_golden_dispatch.py).  ``ir_shared_attn_kernel_name`` formats the very choice the launch
switches on, so equality over the grid - names, refusals and their error texts, under IR_ATTN_W128 unset / 0 / 1 - holds the one
decision to what the two earlier restatements of it answered."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dispatch_grid as DG  # noqa: E402


def test_dispatch_equals_the_golden_record():
    z = np.load(os.path.join(HERE, "golden", "dispatch_golden.npz"))
    table = [tuple(e) for e in json.loads(bytes(z["table"]).decode())]
    entries = list(DG.grid())
    assert z["index"].shape == (len(DG.W128_ENV), len(entries))
    runs = DG.record_in_children()
    for w128, want_idx, got in zip(DG.W128_ENV, z["index"], runs):
        assert len(got) == len(entries)
        bad = [(e, table[i], tuple(g)) for e, i, g in zip(entries, want_idx, got) if table[i] != tuple(g)]
        assert not bad, (f"IR_ATTN_W128={w128}: {len(bad)} of {len(entries)} calls differ; first (call, recorded, now):", bad[:3])
    # the grid reaches every family, the refusals and the batch-invariant names
    names = {n for n, _ in table}
    for part in ("w128_kernel", "w64_kernel<64 rows/wave, 8 waves", "w64_kernel<64 rows/wave, 4 waves", "pipe_kernel", "batch-invariant",
                 "zero suffix in closed form", "segment masses", "forms>"):
        assert any(part in n for n in names), part
    assert ("", "tuning value 5 is not available in this build") in table
