"""Same-box A/B of region-restricted attention (``ops.shared_attention(q_allow=, key_region=)``: the REGION form of the
software-pipelined 32-row kernel) at cfg 2's three shared layer classes (bf16, B 8, N 4: 4096 / 1024 / 256 tokens with 5 / 10 / 20
heads; AdaIN fold, pre-scaled Q, self segment included).  Five sides per class:

  (a) the plain call (default dispatch)
  (b) the bias form with the all-rows mask equivalent to "everything allowed": an all-zero key bias, this build
  (c) the same on the PARENT commit's library (``--parent-lib``: a build of the parent's csrc with IR_BUILD_DIR / IR_OUT pointing
      elsewhere), loaded by a worker process of this tool - the yardstick
  (d) the region form with everything allowed (every key in region 0, every row bit 0)
  (e) the region form with the 4-class rule: a 2 x 2 grid of classes on every picture, own class only, self free

What to read off: (b) against (c) - the bias instantiations are the code they were; (d)/(c) - what the per-element test costs over
the bias form's add (both walk every tile and do the same softmax); (e)/(d) - whether the masked pairs change the time (no tile is
skipped, so they should not).  Each side is ``ir_time_shared_attn_fwd`` (HIP events around 10 back-to-back launches); sides alternate
call by call in a rotating order after a warm-up, for SECS seconds (default 1.5) three times; a side's figure is the median of its
three window means.

usage: python tools/gpu_region_ab.py --parent-lib PATH/libinstantrestore_hip.so [--out profiles/region_ab.txt]"""
import argparse
import datetime
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_kv_table_ab import B, CLASSES, ITERS, N, SCALE, class_data, med, windows  # noqa: E402  (same data, same windows)


def call(L, H, data, **kw):
    from instantrestore_amd import ops
    q, k, v, rk, rv, aff = data
    return lambda: ops.time_shared_attention(q, k, v, rk, rv, heads=H, scale=SCALE, include_self=True, adain=aff, iters=ITERS, q_prescaled=True, **kw)


def zero_bias(L):
    from instantrestore_amd import ops
    return ops.key_bias(B, L, N, L, True, device="cuda")


def worker():
    """the parent commit's library (IR_LIB_PATH, set by the caller): one timed call of side (c) per request line"""
    calls = {}
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        L, H = int(cmd[1]), int(cmd[2])
        if cmd[0] == "setup":
            calls[(L, H)] = call(L, H, class_data(L, H), key_bias=zero_bias(L))
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
    lines = [f"# region-restricted attention, cfg 2 (bf16, B {B}, N {N}, AdaIN fold, pre-scaled Q), same box, sides alternating call by "
             f"call, {secs} s x 3, median of the window means [the three window means]",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}  "
             f"{_lib.lib().ir_build_info().decode()}"]
    for L, H in CLASSES:
        data = class_data(L, H)
        q, k, v, rk, rv, aff = data
        side = int(round(L ** 0.5))
        t = torch.arange(side, device="cuda") * 2 // side
        grid = (t[:, None] * 2 + t[None, :]).reshape(1, L).expand(B, L)                       # a 2 x 2 grid of classes 0 .. 3 on every picture
        everything = (torch.ones(B, L, dtype=torch.int32, device="cuda"), torch.zeros(B, (1 + N) * L, dtype=torch.int32, device="cuda"))
        rule = ops.region_masks(grid, grid.repeat(1, 1 + N), torch.eye(4, dtype=torch.bool), self_len=L, self_free=True)
        kw = dict(heads=H, scale=SCALE, include_self=True, adain=aff, q_prescaled=True)
        lines.append(f"## L {L} H {H}")
        lines.append(f"    plain call       : {ops.shared_attention_kernel_name(q, k, v, rk, rv, **kw)}")
        lines.append(f"    with a bias      : {ops.shared_attention_kernel_name(q, k, v, rk, rv, key_bias=zero_bias(L), **kw)}")
        lines.append(f"    with regions     : {ops.shared_attention_kernel_name(q, k, v, rk, rv, q_allow=rule[0], key_region=rule[1], **kw)}")
        sides = {"a": call(L, H, data), "b": call(L, H, data, key_bias=zero_bias(L)),
                 "d": call(L, H, data, q_allow=everything[0], key_region=everything[1]), "e": call(L, H, data, q_allow=rule[0], key_region=rule[1])}
        if child is not None:
            ask(f"setup {L} {H}")
            lines.append("    worker           : the parent commit's library")
            sides["c"] = lambda: float(ask(f"run {L} {H}"))
        res = windows(sides, secs)
        for n, what in (("a", "plain call"), ("b", "bias form, all-zero bias, this build"), ("c", "the same on the parent's library"),
                        ("d", "region form, everything allowed"), ("e", "region form, 4 classes, own class only, self free")):
            if n in res:
                lines.append(f"({n}) {what:50s}: {fmt(res[n])}")
        y = "c" if "c" in res else "b"
        if "c" in res:
            spread, excess = max(res["c"]) - min(res["c"]), abs(med(res["b"]) - med(res["c"]))
            lines.append(f"(b) vs (c): |b - c| {excess * 1e3:.2f} us, spread of (c) {spread * 1e3:.2f} us: {'met' if excess <= spread else 'MISSED'}   b/c {med(res['b']) / med(res['c']):.4f}")
        spread = max(max(res[n]) - min(res[n]) for n in res)
        lines.append(f"(d)/({y}) {med(res['d']) / med(res[y]):.4f}   (e)/({y}) {med(res['e']) / med(res[y]):.4f}   (e)/(d) {med(res['e']) / med(res['d']):.4f}   "
                     f"(d)/(a) {med(res['d']) / med(res['a']):.4f}   (d) - ({y}) {(med(res['d']) - med(res[y])) * 1e3:.2f} us, largest spread of a side {spread * 1e3:.2f} us")
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
