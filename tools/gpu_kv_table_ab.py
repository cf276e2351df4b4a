"""Same-box A/B of reference K/V read through pointer tables (``ops.RefKVTable``, ``ReferenceKVCache.assemble_tables``) against the
dense ``(B, N, L, C)`` layout, at cfg 2 (bf16, B 8, N 4, 512 px: shared layers of 4096 / 1024 / 256 tokens with 5 / 10 / 20 heads,
three of each; AdaIN fold, pre-scaled Q, self segment included).

  (a) side A: the dense launch on this build      side B: the table launch on this build, same data
  (b) side A: the dense launch on the PARENT commit's library (``--parent-lib``: a build of the parent's csrc with IR_BUILD_DIR /
      IR_OUT pointing elsewhere), loaded by a worker process of this tool      side B: the dense launch on this build
  (c) side A: a nine-layer cached step with ``ReferenceKVCache.assemble()`` inside the timed region
      side B: the same step with ``assemble_tables()``; next to them the bytes ``assemble()`` moved, from the shapes

(a) and (b) are taken per layer class with ``ir_time_shared_attn_fwd`` (HIP events around 10 back-to-back launches) and reported
for the top layer and as the nine-layer sum (3 x the sum of the classes).  Sides alternate call by call in a rotating order (the
worker process answers one timed call per request), after a warm-up, for SECS seconds (default 1.5) three times; a side's figure is the median
of its three window means.  Condition of (a) and (b): the slower side exceeds the faster by no more than the spread (max - min) of
side A's own three window means.  The box's device-to-device copy rate of the same run is written next to (c).

usage: python tools/gpu_kv_table_ab.py --parent-lib PATH/libinstantrestore_hip.so [--out profiles/kv_table_ab.txt]"""
import argparse
import datetime
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = [(4096, 5), (1024, 10), (256, 20)]      # (tokens, heads) of cfg 2's shared layer classes, three layers each
B, N = 8, 4
SCALE, LOG2E = 0.125, 1.4426950408889634
ITERS = 10


def class_data(L, H):
    """the tensors of one shared-attention call, seeded: the same in this process and in the worker"""
    import torch
    from instantrestore_amd import ops
    dt, C = torch.bfloat16, H * 64
    gen = torch.Generator(device="cuda").manual_seed(L + H)
    q = (torch.randn(B, L, C, device="cuda", generator=gen) * (SCALE * LOG2E)).to(dt)
    k, v = (torch.randn(B, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    rk = torch.randn(B, N, L, C, device="cuda", generator=gen).to(dt)
    rv = (torch.randn(B, N, L, C, device="cuda", generator=gen) * 1.2 + 0.3).to(dt)
    return q, k, v, rk, rv, ops.adain_stats(v, rv, heads=H)


def dense_call(L, H, data):
    from instantrestore_amd import ops
    q, k, v, rk, rv, aff = data
    return lambda: ops.time_shared_attention(q, k, v, rk, rv, heads=H, scale=SCALE, include_self=True, adain=aff, iters=ITERS, q_prescaled=True)


def worker():
    """the parent commit's library (IR_LIB_PATH, set by the caller): one timed dense call per request line"""
    calls = {}
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        L, H = int(cmd[1]), int(cmd[2])
        if cmd[0] == "setup":
            calls[(L, H)] = dense_call(L, H, class_data(L, H))
            calls[(L, H)]()
            from instantrestore_amd import _lib
            print("IRAB " + _lib.LIB_PATH, flush=True)
        else:
            print("IRAB " + repr(calls[(L, H)]()), flush=True)


def windows(sides, secs):
    """alternate the sides call by call for `secs` seconds, three times: {side: three window means}.  The order rotates from pass
    to pass (A B C, B C A, ...): a side that always ran behind the same neighbour would inherit that neighbour's cache contents"""
    for fn in sides.values():
        fn()
    res = {n: [] for n in sides}
    order = list(sides)
    for _ in range(3):
        acc = {n: [] for n in sides}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < secs:
            for n in order:
                acc[n].append(sides[n]())
            order = order[1:] + order[:1]
        for n in sides:
            res[n].append(sum(acc[n]) / len(acc[n]))
    return res


def med(x):
    return sorted(x)[1]


def verdict(a, b):
    """side A's three window means against side B's: the condition of (a) and (b)"""
    ma, mb = med(a), med(b)
    spread = max(a) - min(a)
    excess = abs(ma - mb)
    return (f"A {ma * 1e3:8.2f} us  B {mb * 1e3:8.2f} us  B/A {mb / ma:.4f}  |A - B| {excess * 1e3:.2f} us  spread of A {spread * 1e3:.2f} us: "
            f"{'met' if excess <= spread else 'MISSED'}   [A {' '.join(f'{x * 1e3:.2f}' for x in a)} | B {' '.join(f'{x * 1e3:.2f}' for x in b)}]")


def cached_step(secs, lines):
    """(c): nine shared layers through SharedAttnProcessor, the batch's K/V served from a ReferenceKVCache of eight identities"""
    import torch
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd import ops
    from instantrestore_amd.attention import Attention
    from instantrestore_amd.kv_cache import ReferenceKVCache
    dt = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(1)
    shapes = [c for c in CLASSES for _ in range(3)]
    attns, hidden = [], []
    for i, (L, H) in enumerate(shapes):
        torch.manual_seed(i)
        attns.append(Attention(query_dim=H * 64, heads=H, dim_head=64,
                               processor=SharedAttnProcessor(self_attn_idx=i, use_adain=True, train_input=True)).eval().cuda().to(dt))
        hidden.append(torch.randn(B, L, H * 64, device="cuda", generator=gen).to(dt))
    cache = ReferenceKVCache(max_identities=B)

    def identity():
        keys = [torch.randn(1, N, L, H * 64, device="cuda", generator=gen).to(dt) for L, H in shapes]
        values = [(torch.randn(1, N, L, H * 64, device="cuda", generator=gen) * 1.2 + 0.3).to(dt) for L, H in shapes]
        return keys, values, [ops.token_stats(v, heads=H) for v, (L, H) in zip(values, shapes)]

    ids = list(range(B))
    for i in ids:
        cache.get_or_compute(i, identity)

    def step(assemble):
        got = assemble(ids)
        keys, values, stats = got[0], got[1], got[2]
        with torch.no_grad(), torch.autocast("cuda", dtype=dt):
            return [a(h, ref_keys=keys, ref_values=values, ref_stats=stats) for a, h in zip(attns, hidden)]

    for x, y in zip(step(cache.assemble), step(cache.assemble_tables)):
        assert torch.equal(x, y), "the table step differs from the dense step"

    def timed(fn, reps=4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    kv_bytes = sum(2 * B * N * L * H * 64 * 2 for L, H in shapes)
    src = torch.empty(kv_bytes, dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    res = windows({"assemble": lambda: timed(lambda: step(cache.assemble)), "tables": lambda: timed(lambda: step(cache.assemble_tables)),
                   "copy": lambda: timed(lambda: dst.copy_(src))}, secs)
    a, t, c = (med(res[n]) for n in ("assemble", "tables", "copy"))
    lines.append(f"## (c) nine-layer cached step, eager, {B} identities x {N} references, K/V of the batch {kv_bytes / 1e9:.3f} GB")
    lines.append(f"assemble() inside the step : {a:.4f} ms   [{' '.join(f'{x:.4f}' for x in res['assemble'])}]   "
                 f"(torch.cat reads {kv_bytes / 1e9:.3f} GB and writes {kv_bytes / 1e9:.3f} GB in 18 launches, {kv_bytes / 1e9:.3f} GB allocated per step)")
    lines.append(f"assemble_tables() inside   : {t:.4f} ms   [{' '.join(f'{x:.4f}' for x in res['tables'])}]   "
                 f"(one host-to-device copy of {(18 * B * N + B // 2) * 8} bytes, no K/V-sized allocation)")
    lines.append(f"difference {a - t:+.4f} ms per step ({(a - t) / a * 100:+.1f} %)")
    lines.append(f"device-to-device copy of {kv_bytes / 1e9:.3f} GB on this box, same run: {c:.4f} ms = {2 * kv_bytes / c / 1e9:.2f} TB/s read + written   "
                 f"[{' '.join(f'{x:.4f}' for x in res['copy'])}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libinstantrestore_hip.so built from the parent commit; without it (b) is skipped")
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
    lines = [f"# reference K/V through pointer tables vs the dense layout, cfg 2 (bf16, B {B}, N {N}), same box, sides alternating call by call, "
             f"{secs} s x 3, median of the window means",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}  "
             f"{_lib.lib().ir_build_info().decode()}"]
    per_class = {}
    for L, H in CLASSES:
        data = class_data(L, H)
        q, k, v, rk, rv, aff = data
        tk = ops.RefKVTable.from_tensors([[rk[b, n] for n in range(N)] for b in range(B)])
        tv = ops.RefKVTable.from_tensors([[rv[b, n] for n in range(N)] for b in range(B)])
        kw = dict(heads=H, scale=SCALE, include_self=True, adain=aff, q_prescaled=True)
        name = ops.shared_attention_kernel_name(q, k, v, rk, rv, **kw)
        assert ops.shared_attention_kernel_name(q, k, v, tk, tv, **kw) == name
        assert torch.equal(ops.shared_attention(q, k, v, tk, tv, **kw), ops.shared_attention(q, k, v, rk, rv, **kw)), "table launch differs"
        sides = {"dense": dense_call(L, H, data),
                 "table": lambda: ops.time_shared_attention(q, k, v, tk, tv, iters=ITERS, **kw)}
        if child is not None:
            lib = ask(f"setup {L} {H}")
            sides["parent"] = lambda: float(ask(f"run {L} {H}"))
            lines.append(f"# worker: {lib}")
        per_class[(L, H)] = res = windows(sides, secs)
        lines.append(f"## L {L} H {H}: {name}")
        lines.append("(a) dense (A) vs table (B), this build      : " + verdict(res["dense"], res["table"]))
        if child is not None:
            lines.append("(b) dense on the parent's library (A) vs dense on this build (B): " + verdict(res["parent"], res["dense"]))
        del data, q, k, v, rk, rv, tk, tv, sides
        torch.cuda.empty_cache()
    nine = {n: [3 * sum(per_class[c][n][w] for c in CLASSES) for w in range(3)] for n in per_class[CLASSES[0]]}
    lines.append("## nine shared layers (3 x the sum of the three classes, window by window)")
    lines.append("(a) dense (A) vs table (B), this build      : " + verdict(nine["dense"], nine["table"]))
    if child is not None:
        lines.append("(b) dense on the parent's library (A) vs dense on this build (B): " + verdict(nine["parent"], nine["dense"]))
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    cached_step(secs, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
