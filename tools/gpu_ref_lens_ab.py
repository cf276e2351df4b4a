"""Same-box A/B of the per-reference token counts of the fused attention (``ops.shared_attention(ref_lens=)``: the RAGGED form of the
software-pipelined 32-row kernel) and of ``ops.compact_refs`` at cfg 2's three shared layer classes (bf16, B 8, N 4: 4096 / 1024 / 256
tokens with 5 / 10 / 20 heads; AdaIN fold, pre-scaled Q, self segment included).  Sides per class:

  (a) the default dispatch, no mask (the 128-row kernel at the 64x64-token class)
  (b) ``IR_TUNE_PIPE32_PRESCALE_Q`` (the 32-row kernel's pre-scaled form), no counts, this build
  (c) the same on the PARENT commit's library (``--parent-lib``), loaded by a worker process of this tool
  (d) a counted call with every count equal to len_ref
  (e) / (g) today's way: a bias call carrying a centred elliptical keep mask of area 0.5 / 0.25 of every reference
  (f) / (h) the references compacted under the same mask, and a counted call on them

Three things to read off.  The cost of the form: (d) against (b) on the same build and against (c) - N scalar loads and a scan per
item, one compare per segment; the condition is a difference inside the spread of the window means.  The gain of compaction: (f), (h)
against the bias call with the same mask, against (b), and against (a); the claim is time proportional to
``tiles_self + sum ceil(c / 64)`` against (b).  And the compaction kernel's rate against a copy of the same bytes in the same run.
Each attention side is ``ir_time_shared_attn_fwd`` (HIP events around 10 back-to-back launches); sides alternate call by call in a
rotating order after a warm-up, for SECS seconds (default 1.5) three times; a side's figure is the median of its three window means.

usage: python tools/gpu_ref_lens_ab.py --parent-lib PATH/libinstantrestore_hip.so [--out profiles/ref_lens_ab.txt]"""
import argparse
import datetime
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_kv_table_ab import B, CLASSES, ITERS, N, SCALE, class_data, med, windows  # noqa: E402  (same data, same windows)

PRESC = 11      # IR_TUNE_PIPE32_PRESCALE_Q
FRACTIONS = (0.5, 0.25)


def ellipse_keep(side, fraction):
    """bool (side, side): a centred ellipse (axes 1 : 1.25, a face's) whose area is `fraction` of the square"""
    import math
    import torch
    a = side * math.sqrt(fraction / (1.25 * math.pi))
    y, x = torch.meshgrid(torch.arange(side) + 0.5 - side / 2, torch.arange(side) + 0.5 - side / 2, indexing="ij")
    return (x / a) ** 2 + (y / (1.25 * a)) ** 2 <= 1.0


def call(L, H, data, tuning=0, **extra):
    from instantrestore_amd import ops
    q, k, v, rk, rv, aff = data

    def run():
        prev = ops.set_attn_variant(tuning)
        try:
            return ops.time_shared_attention(q, k, v, rk, rv, heads=H, scale=SCALE, include_self=True, adain=aff, iters=ITERS, q_prescaled=True, **extra)
        finally:
            ops.set_attn_variant(prev)
    return run


def worker():
    """the parent commit's library (IR_LIB_PATH, set by the caller): one timed call of side (c) per request line"""
    from instantrestore_amd import _lib
    _lib.SYMBOLS.pop("ir_compact_ref_tokens", None)      # the parent's library does not have the entry point; side (c) does not use it
    calls = {}
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        L, H = int(cmd[1]), int(cmd[2])
        if cmd[0] == "setup":
            calls[(L, H)] = call(L, H, class_data(L, H), PRESC)
            calls[(L, H)]()
            from instantrestore_amd import _lib
            print("IRAB " + _lib.LIB_PATH, flush=True)
        else:
            print("IRAB " + repr(calls[(L, H)]()), flush=True)


def fmt(x):
    return f"{med(x) * 1e3:9.2f} us  [{' '.join(f'{v * 1e3:.2f}' for v in x)}]"


def time_ms(fn, reps=20):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libinstantrestore_hip.so built from the parent commit; without it (c) is skipped")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker()
    secs = float(os.environ.get("SECS", "1.5"))
    child = None
    if args.parent_lib:      # started before this process touches the GPU
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                 env=dict(os.environ, IR_LIB_PATH=os.path.abspath(args.parent_lib)))

    def ask(msg):
        child.stdin.write(msg + "\n")
        child.stdin.flush()
        while True:      # (anything else the runtime prints on the worker's stdout is skipped)
            ans = child.stdout.readline()
            if not ans:
                raise RuntimeError("the worker process ended")
            if ans.startswith("IRAB "):
                return ans[5:].strip()

    import torch
    from instantrestore_amd import _lib, ops
    lines = [f"# per-reference token counts of the fused attention, cfg 2 (bf16, B {B}, N {N}, AdaIN fold, pre-scaled Q), same box, sides alternating "
             f"call by call, {secs} s x 3, median of the window means [the three window means]",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}  "
             f"{_lib.lib().ir_build_info().decode()}"]
    for L, H in CLASSES:
        data = class_data(L, H)
        q, k, v, rk, rv, aff = data
        side = int(round(L ** 0.5))
        full = torch.full((B, N), L, dtype=torch.int32, device="cuda")
        kw = dict(heads=H, scale=SCALE, include_self=True, adain=aff, q_prescaled=True)
        lines.append(f"## L {L} H {H}")
        lines.append(f"    default, no counts : {ops.shared_attention_kernel_name(q, k, v, rk, rv, **kw)}")
        lines.append(f"    with counts        : {ops.shared_attention_kernel_name(q, k, v, rk, rv, ref_lens=full, **kw)}")
        sides = {"a": call(L, H, data), "b": call(L, H, data, PRESC), "d": call(L, H, data, 0, ref_lens=full)}
        names = [("a", "default dispatch, no mask"), ("b", "32-row pre-scaled form, no counts, this build"), ("c", "the same on the parent's library"),
                 ("d", "counted call, every count = len_ref")]
        tiles = {"b": (L + 63) // 64 * (1 + N)}
        compaction = []
        for frac, (nb, nc) in zip(FRACTIONS, (("e", "f"), ("g", "h"))):
            keep = ellipse_keep(side, frac).reshape(1, 1, L).expand(B, N, L).contiguous().cuda()
            bias = ops.key_bias(B, L, N, L, True, ref_token_keep=keep, device="cuda")
            ck, cv, lens = ops.compact_refs(rk, rv, keep, heads=H)
            c = int(lens[0, 0])
            tiles[nc] = (L + 63) // 64 + N * ((c + 63) // 64)
            sides[nb] = call(L, H, data, 0, key_bias=bias)
            sides[nc] = call(L, H, (q, k, v, ck, cv, aff), 0, ref_lens=lens)
            names += [(nb, f"bias call, elliptical keep mask of area {frac} ({c} of {L} keys kept)"), (nc, f"compacted under the same mask, counted call ({tiles[nc]} tiles)")]
            # the compaction itself against a copy of the same bytes (K and V of every reference), same run
            out = (ck, cv, lens)
            t_c = time_ms(lambda: ops.compact_refs(rk, rv, keep, heads=H, out=out))
            t_m = time_ms(lambda: (ck.copy_(rk), cv.copy_(rv)))
            moved = 2 * 2 * B * N * c * H * 64 * 2          # K and V, read + written, 2 bytes per element
            whole = 2 * 2 * B * N * L * H * 64 * 2
            compaction.append(f"    compact_refs, keep {frac}: {t_c * 1e3:8.1f} us = {moved / t_c / 1e6:7.1f} GB/s of moved bytes;  copy of K and V: {t_m * 1e3:8.1f} us = "
                              f"{whole / t_m / 1e6:7.1f} GB/s")
        if child is not None:
            ask(f"setup {L} {H}")
            lines.append("    worker             : the parent commit's library")
            sides["c"] = lambda: float(ask(f"run {L} {H}"))
        res = windows(sides, secs)
        for n, what in names:
            if n in res:
                lines.append(f"({n}) {what:72s}: {fmt(res[n])}")
        spread_b = max(res["b"]) - min(res["b"])
        excess = abs(med(res["d"]) - med(res["b"]))
        lines.append(f"(d) vs (b): |d - b| {excess * 1e3:.2f} us, spread of (b) {spread_b * 1e3:.2f} us: {'inside' if excess <= spread_b else 'OUTSIDE'}   d/b {med(res['d']) / med(res['b']):.4f}")
        if "c" in res:
            spread, ex_b, ex_d = max(res["c"]) - min(res["c"]), abs(med(res["b"]) - med(res["c"])), abs(med(res["d"]) - med(res["c"]))
            lines.append(f"(b) vs (c): |b - c| {ex_b * 1e3:.2f} us, spread of (c) {spread * 1e3:.2f} us: {'inside' if ex_b <= spread else 'OUTSIDE'}   b/c {med(res['b']) / med(res['c']):.4f}"
                         f"   (d) vs (c): d/c {med(res['d']) / med(res['c']):.4f} ({'inside' if ex_d <= spread else 'OUTSIDE'})")
        for frac, (nb, nc) in zip(FRACTIONS, (("e", "f"), ("g", "h"))):
            lines.append(f"keep {frac}: compacted/bias ({nc})/({nb}) {med(res[nc]) / med(res[nb]):.4f}   compacted/unragged ({nc})/(b) {med(res[nc]) / med(res['b']):.4f} "
                         f"(tiles {tiles[nc]}/{tiles['b']} = {tiles[nc] / tiles['b']:.4f})   compacted/default ({nc})/(a) {med(res[nc]) / med(res['a']):.4f}   "
                         f"bias/default ({nb})/(a) {med(res[nb]) / med(res['a']):.4f}")
        lines += compaction
        del data, q, k, v, rk, rv, sides
        torch.cuda.empty_cache()
    if child is not None:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=30)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
