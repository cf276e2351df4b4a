"""Same-box, one-process A/B of the attention rows of chosen query tokens (``ops.attn_rows``) against the only route there was
before it: the whole dump followed by a gather (``ops.attn_probs(...)[:, :, idx]``).

  cfg 2 top shared layer: bf16, B 8, H 5, L = Ls = Lr = 4096, N 4, self included, R = 68 seeded rows with duplicates
  cfg 5 top shared layer at one identity: B 1, L = 16384 (the dump would be 13.4 GB: not run, its bytes are written down)

  (a) dump + gather (cfg 2 only), eager, HIP events around 4 back-to-back repetitions
  (b) attn_rows in each of the three forms, 20 calls captured in one graph, events around a replay (the call's host side
      - argument checks, the output allocation - would otherwise hide a kernel of tens of microseconds)
  (c) a device-to-device copy that moves as many bytes as (b) does (K read once + the output written: a copy of half that
      many bytes reads and writes the total), the same way: the rate the box gives on that day

Sides alternate ((a) b0 b1 b2 c0 c1 c2, repeated for SECS seconds, default 1.5, three times; the median of the three).
``--test-log FILE``: the output of ``pytest -s tests/test_gpu_attn_rows.py``; its "vs oracle" lines are folded into the
maxima per form and dtype.   usage: python tools/gpu_attn_rows_ab.py [--out FILE] [--test-log FILE]"""
import argparse
import datetime
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantrestore_amd import ops  # noqa: E402

FORMS = ("none", "head_mean", "map")
CALLS_PER_GRAPH = 20


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(CALLS_PER_GRAPH)]
    return g, keep


def layer(B, H, L, N, secs, with_dump, lines):
    C = H * 64
    dt = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(B, L, C, device="cuda", generator=gen) * 1.2).to(dt)
    k, v = (torch.randn(B, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    rk, rv = (torch.randn(B, N, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    _, lse = ops.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True)
    del v, rv
    R = 68
    rng = np.random.default_rng(0)
    idx = rng.integers(0, L, size=(B, R))
    idx[:, 1], idx[:, -1] = idx[:, 0], idx[:, 2]
    idx = torch.from_numpy(idx.astype(np.int32)).cuda()
    idxl = idx.long()
    lkv = (N + 1) * L
    kbytes = B * H * lkv * 64 * 2
    obytes = {"none": B * H * R * lkv * 2, "head_mean": B * R * lkv * 4, "map": B * lkv * 4}
    dump_bytes = B * H * L * lkv * 2
    lines.append(f"## B {B} H {H} L {L} N {N} R {R} bf16: K {kbytes / 1e6:.1f} MB, dump {dump_bytes / 1e9:.2f} GB, "
                 + ", ".join(f"{f} {obytes[f] / 1e6:.2f} MB" for f in FORMS))

    kw = dict(heads=H, scale=0.125, include_self=True)
    sides = {}
    if with_dump:
        def dump_gather():
            p = ops.attn_probs(q, k, rk, lse, **kw)
            return torch.stack([p[b][:, idxl[b]] for b in range(B)])
        ref = dump_gather()
        assert torch.equal(ref, ops.attn_rows(q, k, rk, lse, idx, reduce="none", **kw)), "form none differs from the dump's rows"
        del ref
        sides["a"] = lambda: timed(dump_gather, 4)
    graphs = {}
    for f in FORMS:
        graphs["b_" + f] = graph_of(lambda f=f: ops.attn_rows(q, k, rk, lse, idx, reduce=f, **kw))
        n = (kbytes + obytes[f]) // 2 // 16 * 16
        src = torch.empty(n, dtype=torch.uint8, device="cuda").random_()
        dst = torch.empty_like(src)
        graphs["c_" + f] = graph_of(lambda src=src, dst=dst: dst.copy_(src))
    for name, (g, _keep) in graphs.items():
        sides[name] = lambda g=g: timed(g.replay, 3) / CALLS_PER_GRAPH
    for fn in sides.values():
        fn()
    meds = {}
    for _ in range(3):
        acc = {n: [] for n in sides}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < secs:
            for n, fn in sides.items():
                acc[n].append(fn())
        for n in sides:
            meds.setdefault(n, []).append(float(np.mean(acc[n])))
    ms = {n: sorted(x)[1] for n, x in meds.items()}
    if with_dump:
        lines.append(f"(a) attn_probs + probs[:, :, idx]: {ms['a']:.4f} ms   [{' '.join(f'{x:.4f}' for x in meds['a'])}]")
    else:
        lines.append(f"(a) not run: the dump would need {dump_bytes / 1e9:.2f} GB per identity")
    for f in FORMS:
        tb, tc = ms["b_" + f], ms["c_" + f]
        moved = kbytes + obytes[f]
        line = (f"(b) attn_rows {f:9s}: {tb * 1e3:8.1f} us  {moved / tb / 1e9:6.2f} TB/s of K + output   "
                f"(c) copy moving the same bytes: {tc * 1e3:8.1f} us  {moved / tc / 1e9:6.2f} TB/s   fraction of the copy rate {tc / tb:.3f}")
        if with_dump:
            line += f"   (a)/(b) {ms['a'] / tb:.1f}x (required >= 5x: {'met' if ms['a'] / tb >= 5 else 'MISSED'})"
        lines.append(line + f"   [b {' '.join(f'{x * 1e3:.1f}' for x in meds['b_' + f])} | c {' '.join(f'{x * 1e3:.1f}' for x in meds['c_' + f])}]")
    del graphs, sides
    torch.cuda.empty_cache()


def fold_test_log(path, lines):
    pat = re.compile(r"attn_rows .*?(float16|bfloat16|bf16).*?vs (?:oracle|float64) none (\S+) head_mean (\S+) map (\S+)")
    best = {}
    for ln in open(path, errors="replace"):
        m = pat.search(ln)
        if m:
            dt = "fp16" if m.group(1) == "float16" else "bf16"
            cur = best.setdefault(dt, [0.0, 0.0, 0.0, 0])
            for i in range(3):
                cur[i] = max(cur[i], float(m.group(2 + i)))
            cur[3] += 1
    lines.append("## max deviation from the float64 oracle in tests/test_gpu_attn_rows.py (bounds: 1e-3 fp16 / 8e-3 bf16 for none and head_mean, R x that for map)")
    for dt, (e0, e1, e2, n) in sorted(best.items()):
        lines.append(f"{dt}: none {e0:.3e}  head_mean {e1:.3e}  map {e2:.3e}   ({n} sets of rows)")
    if not best:
        lines.append("(no 'vs oracle' lines in the log)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--test-log", default=None)
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.5"))
    lines = [f"# attention rows of 68 chosen tokens: attn_rows vs dump + gather, same box, one process, alternating, {secs} s x 3, median",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}"]
    layer(8, 5, 4096, 4, secs, True, lines)
    layer(1, 5, 16384, 4, secs, False, lines)
    if args.test_log:
        fold_test_log(args.test_log, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
