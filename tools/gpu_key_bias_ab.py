"""Same-box A/B of the additive key bias of the fused attention (``ops.shared_attention(key_bias=)``: the BIAS form of the
software-pipelined 32-row kernel) at cfg 2's three shared layer classes (bf16, B 8, N 4: 4096 / 1024 / 256 tokens with 5 / 10 / 20
heads; AdaIN fold, pre-scaled Q, self segment included).  Five sides per class:

  (a) the default dispatch, no bias
  (b) ``IR_TUNE_PIPE32_PRESCALE_Q`` (the 32-row kernel's pre-scaled form), no bias, this build
  (c) the same on the PARENT commit's library (``--parent-lib``: a build of the parent's csrc with IR_BUILD_DIR / IR_OUT pointing
      elsewhere), loaded by a worker process of this tool
  (d) a bias call with an all-zero bias
  (e) a bias call with one of the four references masked

Two things to read off: (b) against (c) - the untouched instantiations cost nothing (condition: they differ by no more than the
spread of (c)'s own window means) - and what the bias costs: (d)/(b) over the same kernel, (d)/(a) against the default dispatch
(at the 64x64-token class that is the 128-row kernel).  Each side is ``ir_time_shared_attn_fwd`` (HIP events around 10 back-to-back
launches); sides alternate call by call in a rotating order after a warm-up, for SECS seconds (default 1.5) three times; a side's
figure is the median of its three window means.

usage: python tools/gpu_key_bias_ab.py --parent-lib PATH/libinstantrestore_hip.so [--out profiles/key_bias_ab.txt]"""
import argparse
import datetime
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_kv_table_ab import B, CLASSES, ITERS, N, SCALE, class_data, med, windows  # noqa: E402  (same data, same windows)

PRESC = 11      # IR_TUNE_PIPE32_PRESCALE_Q


def call(L, H, data, tuning=0, bias=None):
    from instantrestore_amd import ops
    q, k, v, rk, rv, aff = data

    def run():
        prev = ops.set_attn_variant(tuning)
        try:
            return ops.time_shared_attention(q, k, v, rk, rv, heads=H, scale=SCALE, include_self=True, adain=aff, iters=ITERS, q_prescaled=True,
                                             key_bias=bias)
        finally:
            ops.set_attn_variant(prev)
    return run


def worker():
    """the parent commit's library (IR_LIB_PATH, set by the caller): one timed call of side (c) per request line"""
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
    lines = [f"# additive key bias of the fused attention, cfg 2 (bf16, B {B}, N {N}, AdaIN fold, pre-scaled Q), same box, sides alternating call by "
             f"call, {secs} s x 3, median of the window means [the three window means]",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}  "
             f"{_lib.lib().ir_build_info().decode()}"]
    for L, H in CLASSES:
        data = class_data(L, H)
        q, k, v, rk, rv, aff = data
        zero = ops.key_bias(B, L, N, L, True, device="cuda")
        w = torch.ones(B, N)
        w[:, 2] = 0.0
        masked = ops.key_bias(B, L, N, L, True, ref_weights=w, device="cuda")
        kw = dict(heads=H, scale=SCALE, include_self=True, adain=aff, q_prescaled=True)
        lines.append(f"## L {L} H {H}")
        lines.append(f"    default, no bias : {ops.shared_attention_kernel_name(q, k, v, rk, rv, **kw)}")
        lines.append(f"    with a bias      : {ops.shared_attention_kernel_name(q, k, v, rk, rv, key_bias=zero, **kw)}")
        sides = {"a": call(L, H, data), "b": call(L, H, data, PRESC), "d": call(L, H, data, 0, zero), "e": call(L, H, data, 0, masked)}
        if child is not None:
            ask(f"setup {L} {H}")
            lines.append("    worker           : the parent commit's library")
            sides["c"] = lambda: float(ask(f"run {L} {H}"))
        res = windows(sides, secs)
        for n, what in (("a", "default dispatch, no bias"), ("b", "32-row pre-scaled form, no bias, this build"), ("c", "the same on the parent's library"),
                        ("d", "bias call, all-zero bias"), ("e", "bias call, reference 2 of 4 masked")):
            if n in res:
                lines.append(f"({n}) {what:46s}: {fmt(res[n])}")
        if "c" in res:
            spread, excess = max(res["c"]) - min(res["c"]), abs(med(res["b"]) - med(res["c"]))
            lines.append(f"(b) vs (c): |b - c| {excess * 1e3:.2f} us, spread of (c) {spread * 1e3:.2f} us: {'met' if excess <= spread else 'MISSED'}   b/c {med(res['b']) / med(res['c']):.4f}")
        lines.append(f"(d)/(b) {med(res['d']) / med(res['b']):.4f}   (d)/(a) {med(res['d']) / med(res['a']):.4f}   (e)/(d) {med(res['e']) / med(res['d']):.4f}")
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
