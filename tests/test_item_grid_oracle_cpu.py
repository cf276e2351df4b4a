"""The reference of the item-grid tests, without a GPU: tests/item_grid_oracle.py agrees with the oracle's own probability
matrix, and the 1e-3 gate of tests/test_gpu_item_grid.py bites - every fault of the (xcd, item, piece) -> (b, h, query block) map
that the gate is there for moves the reference by more than twice the gate in EVERY row it touches (so a kernel that is within
1e-3 of the faulty result cannot also be within 1e-3 of the right one).  Set A's data (bf16-rounded, 384 + 2 x 320 keys) at B = 2,
without AdaIN; the figure asserted on is the minimum over the touched (b, h, row) of the row's max |difference| over its 64
channels.  On this file's seeded data: lost tile 2.1e-2, eight lost keys 2.4e-3 (the one fault near the limit: eight of 1024 keys are the
least a 1e-3 gate can be asked to see), swapped heads 0.14, swapped entries 0.13, rows of the wrong query block 0.11."""
import numpy as np
import pytest
import torch

import item_grid_oracle as G
from oracle import shared_attn_oracle as O

GATE = 1e-3


def test_helper_lse_and_masses_agree_with_the_oracles_probabilities():
    rng = np.random.default_rng(11)
    B, H, Lq, Ls, N, Lr = 2, 3, 37, 41, 3, 29                     # nothing aligned to anything
    q, k, v = rng.standard_normal((B, Lq, H * 64)), rng.standard_normal((B, Ls, H * 64)), rng.standard_normal((B, Ls, H * 64))
    rk, rv = rng.standard_normal((B, N, Lr, H * 64)), rng.standard_normal((B, N, Lr, H * 64)) * 1.4 - 0.2
    for inc in (True, False):
        for adain in (True, False):
            out_ref, p = O.shared_attention_np(q, k, v, rk, rv, H, G.SCALE, adain, inc, return_probs=True)
            out, lse, mass = G.reference(q, k, v, rk, rv, H, G.SCALE, adain, inc)
            assert np.abs(out - out_ref).max() <= 1e-12
            edges = [0] + ([Ls] if inc else []) + [(Ls if inc else 0) + (n + 1) * Lr for n in range(N)]
            m_ref = np.stack([p[..., a:b].sum(-1) for a, b in zip(edges[:-1], edges[1:])], axis=-1)
            assert mass.shape == m_ref.shape and np.abs(mass - m_ref).max() <= 1e-12
            # the oracle's log-sum-exp, out of its probabilities: p = exp(s - lse) at each row's largest score
            kk = np.concatenate(([k] if inc else []) + [rk[:, n] for n in range(N)], axis=1)
            s = np.einsum("blhd,bkhd->bhlk", q.reshape(B, Lq, H, 64), kk.reshape(B, -1, H, 64)) * G.SCALE
            j = s.argmax(-1)[..., None]
            lse_ref = (np.take_along_axis(s, j, -1) - np.log(np.take_along_axis(p, j, -1)))[..., 0]
            assert lse.shape == lse_ref.shape and np.abs(lse - lse_ref).max() <= 1e-12


@pytest.fixture(scope="module")
def set_a():
    inc, Ls, N, Lr, _ = G.FORMS["self+fold"]
    _, H, Lq, rows = G.SETS["A"]
    q, _, k, v, rk, rv = (G.np64(t) for t in G.set_inputs("A", "self+fold", torch.bfloat16, "cpu", batch=2))
    # without AdaIN the extended sequence is one plain attention over [self, reference 0, reference 1]
    kk = np.concatenate([k] + [rk[:, n] for n in range(N)], axis=1)
    vv = np.concatenate([v] + [rv[:, n] for n in range(N)], axis=1)
    ref = O.shared_attention_np(q, k, v, rk, rv, H, G.SCALE, False, inc)
    assert np.abs(O.shared_attention_np(q, kk, vv, None, None, H, G.SCALE) - ref).max() <= 1e-12
    ref.setflags(write=False)
    return q, kk, vv, ref, H, Lq, rows, Ls + Lr          # ... and the first key of reference 1


def _row_moves(a, b, H):
    """max |a - b| over the 64 channels of each (b, row, head)"""
    return np.abs(a - b).reshape(a.shape[0], a.shape[1], H, 64).max(-1)


@pytest.mark.parametrize("lost", [64, 8], ids=["one_tile", "eight_keys"])
def test_lost_keys_of_reference_1_move_every_row_past_twice_the_gate(set_a, lost):
    q, kk, vv, ref, H, _, _, r1 = set_a
    keep = np.r_[0:r1 + 64, r1 + 64 + lost:kk.shape[1]]            # the second tile of reference 1, or its first eight keys
    mut = O.shared_attention_np(q, kk[:, keep], vv[:, keep], None, None, H, G.SCALE)
    moved = _row_moves(mut, ref, H).min()
    print(f"{lost} lost keys: min over rows of the row max {moved:.2e}")
    assert moved > 2 * GATE


def test_swapped_heads_entries_and_query_blocks_move_every_row_past_twice_the_gate(set_a):
    _, _, _, ref, H, Lq, rows, _ = set_a
    heads = ref.copy().reshape(2, Lq, H, 64)
    heads[0, :, [0, 1]] = heads[0, :, [1, 0]]                     # heads 0 and 1 of entry 0
    moved = _row_moves(heads.reshape(ref.shape), ref, H)[0, :, :2].min()
    print(f"two heads swapped: {moved:.2e}")
    assert moved > 2 * GATE
    moved = _row_moves(ref[::-1], ref, H).min()                   # the two entries
    print(f"two entries swapped: {moved:.2e}")
    assert moved > 2 * GATE
    block = ref.copy()
    block[:, rows:] = ref[:, :Lq - rows]                          # rows 512 ... 599 computed from query block 0's rows
    moved = _row_moves(block, ref, H)[:, rows:].min()
    print(f"rows {rows}...{Lq - 1} from query block 0: {moved:.2e}")
    assert moved > 2 * GATE
