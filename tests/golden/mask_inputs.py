"""Seeded inputs of the attention-mask golden cases: the layers of ``f1_inputs`` that a padded-text mask reaches, with an additive
``attention_mask`` - cross attention (128 query rows x 77 text tokens, H = 5) with the last 20 keys at -10000 (what diffusers'
UNet hands the cross-attention layers as ``encoder_attention_mask``), and a plain self-attention (L = 96, H = 2) with soft values
and scattered masked keys.  Shared by the generator (runs the imported reference) and the tests; the fixture holds outputs only."""
import torch

import f1_inputs as FI

CASES = [
    dict(id="mx320h5", kind="cross", C=320, H=5, lowp="bf16", padded=20),
    dict(id="ms96h2", kind="self", L=96, C=128, H=2, lowp="bf16"),
]


def build(meta):
    """-> the ``f1_inputs`` tensors of the case plus ``mask`` (B, 1, Lkv), additive fp32"""
    d = FI.build(meta, seed_base=7700)
    g = torch.Generator().manual_seed(7700 + len(meta["id"]))
    lkv = FI.TEXT if meta["kind"] == "cross" else meta["L"]
    mask = torch.zeros(1, 1, lkv)
    if meta["kind"] == "cross":
        mask[:, :, lkv - meta["padded"]:] = -10000.0
    else:
        mask.copy_(torch.rand(1, 1, lkv, generator=g) * 4 - 2)
        mask[:, :, torch.randperm(lkv, generator=g)[: lkv // 4]] = -10000.0
    d["mask"] = mask
    return d


def checksum(d) -> float:
    t = d["mask"].double().flatten()
    return FI.checksum(d) + float((t * torch.arange(1, t.numel() + 1, dtype=torch.float64)).sum())
