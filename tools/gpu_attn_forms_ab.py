"""Sustained same-box A/B of the 128-row kernel's valid_refs / seg_mass forms (tuning 16) against the 64-row kernel in 8-wave
workgroups (tuning 13) at the top layers (pre-scaled Q, bf16, AdaIN on, remainder split with the library's workspace):

  (a) cfg 2 top layer: B 8, H 5, L 4096, N 4, valid counts [4,3,2,1,4,3,2,1]
  (b) (a) + the segment masses (return_mass)
  (c) cfg 4 top layer: B 8, H 5, L 4096, N 8, 4 of 8 valid         (c-all) the same with all 8 valid, for the per-tile rate
  (a-plain) (a) without valid_refs / masses: the default instantiation, for the by-product's cost

Each figure: back-to-back launches for SECS seconds (default 1.5), three times, the median; tunings alternate inside a case so
both see the same clocks.  usage: python tools/gpu_attn_forms_ab.py [--out FILE]   (SECS=<s> in the environment)"""
import argparse
import datetime
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from instantrestore_amd import ops  # noqa: E402

QC = 0.125 * 1.4426950408889634


def sustained(kw, secs):
    ops.time_shared_attention(**kw, iters=3)
    res = []
    for _ in range(3):
        t0, tot, n = time.perf_counter(), 0.0, 0
        while time.perf_counter() - t0 < secs:
            tot += ops.time_shared_attention(**kw, iters=20) * 20
            n += 20
        res.append(tot / n)
    return sorted(res)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.5"))
    torch.manual_seed(0)
    B, H, L = 8, 5, 4096
    C = H * 64
    lines = [f"# 128-row kernel forms (tuning 16) vs 64-row kernel, 8 waves (tuning 13): sustained same-box A/B, {secs} s x 3, median",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}",
             "# bf16, pre-scaled Q, AdaIN fold, self segment, workspace given (remainder split as in the product)"]
    q = (torch.randn(B, L, C, device="cuda") * QC).to(torch.bfloat16)
    k, v = (torch.randn(B, L, C, device="cuda").to(torch.bfloat16) for _ in range(2))
    rows = {}
    for tag, N, valid, mass in (("a", 4, [4, 3, 2, 1, 4, 3, 2, 1], False), ("b", 4, [4, 3, 2, 1, 4, 3, 2, 1], True),
                                ("a-plain", 4, None, False), ("c", 8, [4] * 8, False), ("c-all", 8, [8] * 8, False)):
        rk = torch.randn(B, N, L, C, device="cuda").to(torch.bfloat16)
        rv = torch.randn(B, N, L, C, device="cuda").to(torch.bfloat16)
        vt = None
        if valid is not None:
            vt = torch.tensor(valid, dtype=torch.int32, device="cuda")
            ops.zero_invalid_refs(rk, rv, vt, heads=H)
        aff = ops.adain_stats(v, rv, heads=H)
        kw = dict(q=q, k_self=k, v_self=v, ref_k=rk, ref_v=rv, heads=H, scale=0.125, include_self=True, adain=aff, q_prescaled=True,
                  valid_refs=vt, return_mass=mass)
        ms = {}
        for t in (16, 13, 16, 13):
            ops.set_attn_variant(t)
            ms.setdefault(t, []).append(sustained(kw, secs))
        ops.set_attn_variant(0)
        m16, m13 = min(ms[16]), min(ms[13])
        rows[tag] = (m16, m13)
        tiles = B * H * (L // 512) * (L // 64) * (1 + (sum(valid) / B if valid is not None else N))
        lines.append(f"({tag:7s}) N {N} valid {valid if valid is not None else 'all (no valid_refs)'} mass {int(mass)}: "
                     f"t16 {m16:.4f} ms  t13 {m13:.4f} ms  t16/t13 {m16 / m13:.3f}   t16 per 1000 item-tiles {1000 * m16 / tiles * 1e3:.3f} us "
                     f"[runs t16 {' '.join(f'{x:.4f}' for x in ms[16])} | t13 {' '.join(f'{x:.4f}' for x in ms[13])}]")
        del rk, rv
    a16, b16, p16 = rows["a"][0], rows["b"][0], rows["a-plain"][0]
    lines.append(f"# mass by-product on tuning 16: (b)/(a) = {b16 / a16:.3f}")
    lines.append(f"# (a) with valid counts vs (a-plain) all valid, tuning 16: {a16 / p16:.3f} of the time for "
                 f"{(1 + 2.5) / (1 + 4):.3f} of the tiles")
    c16, call16 = rows["c"][0], rows["c-all"][0]
    lines.append(f"# (c) per-tile rate against all-valid, tuning 16: {(c16 / (1 + 4)) / (call16 / (1 + 8)):.3f} (1.000 = same rate)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
