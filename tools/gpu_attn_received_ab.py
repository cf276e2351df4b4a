"""Same-box A/B of the key-side read-out (``ops.attn_received``) against the routes there were before it and against its siblings, bf16:

  cfg 2's three classes (B 8, N 4, self included): H 20 L 256, H 10 L 1024, H 5 L 4096; and the 1024-px top layer at one identity
  (B 1, H 5, L 16384, N 4; the dump would be 13.4 GB: routes (a) and (b) are not run there)
    (a) attn_probs, then ``sum(dim=-2)`` of the dump in fp32 - the only route to the received attention there was - and, for weighted
        calls, the dump (converted to fp32, as the weights are) transposed times the weights, per head
    (b) attn_probs alone, the part of (a) that no arrangement of its second half removes
    (c) attn_segment_mass: the same contraction and exponentials, row sums instead of the dump
    (d) attn_transfer per head, all rows, with the same channel count: the transposed walk
    (e) attn_received without weights ("0 ch": plain column sums, no weight is loaded) and with 1 / 2 / 4 / 8 weighted channels,
        both forms; route (a) of the unweighted and of the 1-channel call is the same ``sum(dim=-2)`` / one-column product
  and a device-to-device copy of 1 GiB in the same run (read + write bytes per second).

(c), (d) and (e) are measured as CALLS_PER_GRAPH calls captured in one graph with events around replays (the host side of a call would
otherwise hide a kernel of tens of microseconds); (a) and (b) as a whole eagerly, events around 4 back-to-back repetitions.  Sides
alternate, repeated for SECS seconds (default 1.0), three times; the median of the three.

Every step that touches the GPU is a child process of its own under its own time limit, and the steps are chained: the first one
that fails or runs out of time ends the run (nothing more is started on a device that has just misbehaved).
usage: python tools/gpu_attn_received_ab.py [--out FILE]"""
import argparse
import datetime
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from gpu_attn_transfer_ab import CALLS_PER_GRAPH, graph_of, measure, timed  # noqa: E402

FORMS = ("none", "head_mean")
CHANNELS = (1, 2, 4, 8)
E_CHANNELS = (0,) + CHANNELS   # 0: weights=None
SHAPES = {"c256": (8, 20, 256, 4), "c1024": (8, 10, 1024, 4), "top": (8, 5, 4096, 4), "px1024": (1, 5, 16384, 4)}
STEPS = [                      # (name, child arguments, time limit in seconds)
    ("16x16-token class", ["--step", "c256"], 240),
    ("32x32-token class", ["--step", "c1024"], 240),
    ("64x64-token class", ["--step", "top"], 300),
    ("1024-px layer, one identity", ["--step", "px1024"], 300),
]


def child(step, secs):
    import torch
    from instantrestore_amd import ops
    B, H, L, N = SHAPES[step]
    C, S, dt = H * 64, N + 1, torch.bfloat16
    lkv = S * L
    dump = step != "px1024"
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(B, L, C, device="cuda", generator=gen) * 1.2).to(dt)
    k, v = (torch.randn(B, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    rk, rv = (torch.randn(B, N, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    del v, rv
    w8 = torch.rand(B, L, 8, device="cuda", generator=gen) * 2 - 1                       # a signed map per query token
    y8 = torch.rand(B, lkv, 8, device="cuda", generator=gen) * 2 - 1                     # the transfer's payload of the same width
    wc = {c: w8[..., :c].contiguous() for c in CHANNELS}
    yc = {c: y8[..., :c].contiguous() for c in CHANNELS}
    flops = 2.0 * B * H * L * lkv * 64
    dump_bytes = B * H * L * lkv * 2
    out = [f"## B {B} H {H} L {L} N {N} bf16: {flops / 1e9:.1f} GFLOP of QK^T, dump {dump_bytes / 1e9:.2f} GB"
           f"   (device: {torch.cuda.get_device_name(0)}, torch {torch.__version__})"]
    graphs, sides = {}, {}
    graphs["c"] = graph_of(lambda: ops.attn_segment_mass(q, k, rk, lse, **kw))
    for c in CHANNELS:
        graphs[f"d{c}"] = graph_of(lambda c=c: ops.attn_transfer(q, k, rk, lse, yc[c], None, reduce="none", **kw))
    for c in E_CHANNELS:
        for f in FORMS:
            graphs[f"e{c}_{f}"] = graph_of(lambda c=c, f=f: ops.attn_received(q, k, rk, lse, wc[c] if c else None, reduce=f, **kw))
    if dump:
        def dump_route(c):
            p = ops.attn_probs(q, k, rk, lse, **kw)
            if c == 0:
                return p.sum(dim=-2, dtype=torch.float32)
            return p.float().transpose(-1, -2) @ wc[c][:, None]                         # (B, H, Lkv, c)
        # the routes agree: the dump's probabilities carry one bf16 rounding each (2^-9 relative)
        got = ops.attn_received(q, k, rk, lse, None, reduce="none", **kw)[..., 0]
        want = dump_route(0)
        d = float(((want - got).abs() / want).max())
        assert d <= 2.0 ** -9 * 1.05 + 1e-4, f"attn_received and the dump route differ by {d} relative"
        out.append(f"    max |attn_received - dump route| / dump route, unweighted, per head: {d:.3e} (one bf16 rounding per probability: 2.0e-03)")
        del got, want
        torch.cuda.empty_cache()
        for c in E_CHANNELS:
            sides[f"a{c}"] = lambda c=c: timed(lambda: dump_route(c), 4)
        sides["b"] = lambda: timed(lambda: ops.attn_probs(q, k, rk, lse, **kw), 4)
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    sides["copy"] = lambda: timed(lambda: dst.copy_(src), 4)
    for name, (g, _keep) in graphs.items():
        sides[name] = lambda g=g: timed(g.replay, 3) / CALLS_PER_GRAPH
    ms, runs = measure(sides, secs)
    for c in E_CHANNELS:
        for f in FORMS:
            t = ms[f"e{c}_{f}"]
            what = f"{c} ch      " if c else "no weights"
            line = (f"(e) attn_received {what} {f:9s}: {t * 1e3:9.1f} us  {flops / t / 1e9:7.1f} TFLOP/s of QK^T   (e)/(c) {t / ms['c']:.2f}x   "
                    f"(e)/(d) {t / ms[f'd{max(c, 1)}']:.2f}x")
            if dump:
                line += f"   (a)/(e) {ms[f'a{c}'] / t:.2f}x   (b)/(e) {ms['b'] / t:.2f}x"
            out.append(line + "   " + runs(f"e{c}_{f}"))
    out.append(f"(c) attn_segment_mass          : {ms['c'] * 1e3:9.1f} us  {flops / ms['c'] / 1e9:7.1f} TFLOP/s of QK^T   {runs('c')}")
    for c in CHANNELS:
        out.append(f"(d) attn_transfer {c} ch per head : {ms[f'd{c}'] * 1e3:9.1f} us   {runs(f'd{c}')}")
    if dump:
        out.append(f"(b) attn_probs alone           : {ms['b'] * 1e3:9.1f} us  {dump_bytes / ms['b'] / 1e9:6.2f} TB/s written   {runs('b')}")
        for c in E_CHANNELS:
            what = "sum(dim=-2)     " if c == 0 else f"dump^T @ w, {c} ch"
            out.append(f"(a) attn_probs + {what}: {ms[f'a{c}'] * 1e3:9.1f} us   {runs(f'a{c}')}")
    else:
        out.append(f"(a), (b) not run: the dump would need {dump_bytes / 1e9:.2f} GB per identity")
    out.append(f"    device-to-device copy of 1 GiB : {ms['copy'] * 1e3:9.1f} us  {2 * src.numel() * 4 / ms['copy'] / 1e9:6.2f} TB/s read + written   {runs('copy')}")
    print("\n".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(SHAPES), help="(internal) run one measuring step in this process")
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.0"))
    if args.step is not None:
        child(args.step, secs)
        return 0
    lines = [f"# attention received per key: attn_received vs dump + column sums, attn_probs alone, attn_segment_mass and attn_transfer; same box, "
             f"one process per step, alternating, {secs} s x 3, median",
             f"# date: {datetime.date.today().isoformat()}"]
    rc = 0
    for name, extra, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"## {name}: no result within {limit} s - the run ends here")
            rc = 124
            break
        if r.returncode != 0:
            lines.append(f"## {name}: exit status {r.returncode} - the run ends here")
            lines += ["    " + ln for ln in r.stderr.strip().splitlines()[-8:]]
            rc = r.returncode
            break
        lines += r.stdout.strip().splitlines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
