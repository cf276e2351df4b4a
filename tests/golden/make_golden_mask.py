#!/usr/bin/env python3 -B
"""Golden vectors of the attention-mask path, produced by RUNNING THE REFERENCE (build container only; data only is committed):
the imported reference's ``AttnProcessor`` and ``SharedAttnProcessor(self_attn_idx=None)`` with an additive ``attention_mask``,
through the stand-in ``Attention`` (whose ``prepare_attention_mask`` repeats the mask over the heads and whose
``get_attention_scores`` adds it to the scaled scores, ``baddbmm`` with ``beta = 1``), on the cases of ``mask_inputs``.
Stored: the reference's fp32 output (identical for the two processors, asserted here) and its own 16-bit output.

Run:  python -B tests/golden/make_golden_mask.py   ->  tests/golden/attn_mask_golden.npz
"""
import copy
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("IR_REFERENCE_ROOT", "/root/reference")

import numpy as np
import torch

sys.path.insert(0, REFERENCE)
import face_replace.models.attn_processors as ref_ap  # noqa: E402  (the reference)

assert ref_ap.__file__.startswith(REFERENCE), ref_ap.__file__
sys.path.append(REPO)
sys.path.append(HERE)
from instantrestore_amd.attention import Attention  # noqa: E402  (diffusers stand-in)
import f1_inputs as FI  # noqa: E402
import mask_inputs as MI  # noqa: E402


def make_attn(meta, d):
    attn = Attention(query_dim=meta["C"], cross_attention_dim=FI.CROSS if meta["kind"] == "cross" else None, heads=meta["H"], dim_head=64)
    with torch.no_grad():
        attn.to_q.weight.copy_(d["wq"]); attn.to_k.weight.copy_(d["wk"]); attn.to_v.weight.copy_(d["wv"])
        attn.to_out[0].weight.copy_(d["wo"]); attn.to_out[0].bias.copy_(d["bo"])
    return attn


def run(proc, d, attn, cast):
    with torch.no_grad():
        return proc(attn, cast(d["hidden"]), encoder_hidden_states=cast(d["encoder"]) if "encoder" in d else None,
                    attention_mask=cast(d["mask"]))


def main():
    torch.set_num_threads(8)
    blob, manifest = {}, []
    for meta in MI.CASES:
        d = MI.build(meta)
        attn = make_attn(meta, d)
        plain = run(ref_ap.AttnProcessor(), d, attn, lambda t: t)[0]
        shared = run(ref_ap.SharedAttnProcessor(self_attn_idx=None), d, attn, lambda t: t)[0]
        with torch.no_grad():
            unmasked = ref_ap.AttnProcessor()(attn, d["hidden"], encoder_hidden_states=d.get("encoder"))[0]
        dt = FI.TORCH_DT[meta["lowp"]]
        lo = run(ref_ap.SharedAttnProcessor(self_attn_idx=None), d, copy.deepcopy(attn).to(dt), lambda t: t.to(dt))[0].float()
        assert torch.equal(plain, shared)     # the two reference processors run the same arithmetic here: one output is stored for both
        m = dict(meta, checksum=MI.checksum(d), mask_effect=float((plain - unmasked).abs().max()), processors_agree=True)
        manifest.append(m)
        blob[f"{m['id']}/out"] = plain.detach().numpy().astype(np.float32)
        blob[f"{m['id']}/out_lowp"] = lo.numpy().astype(np.float32)
        print(m["id"], meta["kind"], "max|out|", float(plain.abs().max()), "the two processors differ by", float((plain - shared).abs().max()),
              "mask moves the output by", m["mask_effect"], "ref lowp err", float((lo - plain).abs().max()))
    blob["manifest"] = np.frombuffer(json.dumps(manifest).encode(), dtype=np.uint8)
    out_path = os.path.join(HERE, "attn_mask_golden.npz")
    np.savez_compressed(out_path, **blob)
    print(f"wrote {out_path}: {len(manifest)} cases, {os.path.getsize(out_path) / 1e3:.0f} kB | reference {ref_ap.__file__} | torch {torch.__version__}")


if __name__ == "__main__":
    main()
