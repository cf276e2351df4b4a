"""Same-box A/B of the column maximum (``ops.attn_key_match``) against the route there was before it and against its floor, bf16:

  cfg 2's three classes (B 8, N 4, self included): H 20 L 256, H 10 L 1024, H 5 L 4096; and the 1024-px top layer at one identity
  (B 1, H 5, L 16384, N 4; the dump would be 13.4 GB: routes (a) and (b) are not run there)
    (a) attn_probs, then ``max(dim=-2)`` of the dump (values and indices) - the only route to the column maximum there was; for
        the head mean, ``mean(dim=1)`` of the dump in fp32 first
    (b) attn_probs alone, the part of (a) that no arrangement of its second half removes
    (r) attn_received without weights, both forms: the same K-stationary walk with ONE fused multiply-add per score where the
        column maximum has a compare and two selects - the natural floor
    (k) attn_key_match, both forms
  and a device-to-device copy of 1 GiB in the same run (read + write bytes per second).

(r) and (k) are measured as CALLS_PER_GRAPH calls captured in one graph with events around replays (the host side of a call would
otherwise hide a kernel of tens of microseconds); (a) and (b) as a whole eagerly, events around 4 back-to-back repetitions.  Sides
alternate, repeated for SECS seconds (default 1.0), three times; the median of the three.

Every step that touches the GPU is a child process of its own under its own time limit, and the steps are chained: the first one
that fails or runs out of time ends the run (nothing more is started on a device that has just misbehaved).
usage: python tools/gpu_attn_key_match_ab.py [--out FILE]"""
import argparse
import datetime
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from gpu_attn_transfer_ab import CALLS_PER_GRAPH, graph_of, measure, timed  # noqa: E402

FORMS = ("none", "head_mean")
SHAPES = {"c256": (8, 20, 256, 4), "c1024": (8, 10, 1024, 4), "top": (8, 5, 4096, 4), "px1024": (1, 5, 16384, 4)}
STEPS = [                      # (name, child arguments, time limit in seconds)
    ("16x16-token class", ["--step", "c256"], 180),
    ("32x32-token class", ["--step", "c1024"], 180),
    ("64x64-token class", ["--step", "top"], 240),
    ("1024-px layer, one identity", ["--step", "px1024"], 240),
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
    flops = 2.0 * B * H * L * lkv * 64
    dump_bytes = B * H * L * lkv * 2
    out = [f"## B {B} H {H} L {L} N {N} bf16: {flops / 1e9:.1f} GFLOP of QK^T, dump {dump_bytes / 1e9:.2f} GB"
           f"   (device: {torch.cuda.get_device_name(0)}, torch {torch.__version__})"]
    graphs, sides = {}, {}
    for f in FORMS:
        graphs[f"r_{f}"] = graph_of(lambda f=f: ops.attn_received(q, k, rk, lse, None, reduce=f, **kw))
        graphs[f"k_{f}"] = graph_of(lambda f=f: ops.attn_key_match(q, k, rk, lse, reduce=f, **kw))
    if dump:
        def dump_route(f):
            p = ops.attn_probs(q, k, rk, lse, **kw)
            if f == "head_mean":
                p = p.mean(dim=1, dtype=torch.float32)
            return p.max(dim=-2)
        # the routes agree: per head the call's prob rounded to bf16 IS the dump's column maximum
        got_i, got_p = ops.attn_key_match(q, k, rk, lse, reduce="none", **kw)
        want = dump_route("none")
        assert torch.equal(got_p.to(dt), want.values), "attn_key_match and the dump route differ"
        p = ops.attn_probs(q, k, rk, lse, **kw)
        assert torch.equal(p.gather(-2, got_i.long()[:, :, None, :])[:, :, 0], want.values)
        out.append("    per head: prob rounded to bf16 equals the dump's column maximum, and the dump's element at index attains it")
        del got_i, got_p, want, p
        torch.cuda.empty_cache()
        for f in FORMS:
            sides[f"a_{f}"] = lambda f=f: timed(lambda: dump_route(f), 4)
        sides["b"] = lambda: timed(lambda: ops.attn_probs(q, k, rk, lse, **kw), 4)
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    sides["copy"] = lambda: timed(lambda: dst.copy_(src), 4)
    for name, (g, _keep) in graphs.items():
        sides[name] = lambda g=g: timed(g.replay, 3) / CALLS_PER_GRAPH
    ms, runs = measure(sides, secs)
    for f in FORMS:
        t = ms[f"k_{f}"]
        line = f"(k) attn_key_match {f:9s}: {t * 1e3:9.1f} us  {flops / t / 1e9:7.1f} TFLOP/s of QK^T   (k)/(r) {t / ms[f'r_{f}']:.2f}x"
        if dump:
            line += f"   (a)/(k) {ms[f'a_{f}'] / t:.2f}x   (b)/(k) {ms['b'] / t:.2f}x"
        out.append(line + "   " + runs(f"k_{f}"))
    for f in FORMS:
        t = ms[f"r_{f}"]
        out.append(f"(r) attn_received  {f:9s}: {t * 1e3:9.1f} us  {flops / t / 1e9:7.1f} TFLOP/s of QK^T   {runs(f'r_{f}')}")
    if dump:
        out.append(f"(b) attn_probs alone        : {ms['b'] * 1e3:9.1f} us  {dump_bytes / ms['b'] / 1e9:6.2f} TB/s written   {runs('b')}")
        out.append(f"(a) attn_probs + max(dim=-2), per head         : {ms['a_none'] * 1e3:9.1f} us   {runs('a_none')}")
        out.append(f"(a) attn_probs + mean(dim=1) + max(dim=-2)     : {ms['a_head_mean'] * 1e3:9.1f} us   {runs('a_head_mean')}")
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
    lines = [f"# column maximum per key: attn_key_match vs dump + max(dim=-2), attn_probs alone and attn_received; same box, "
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
