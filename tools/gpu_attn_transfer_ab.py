"""Same-box A/B of the payload read-out (``ops.attn_transfer``) against the routes there were before it, bf16:

  cfg 2's top shared layer: B 8, H 5, L 4096, N 4, self included, all 4096 rows, channels 2 / 4 / 8, both forms
    (t) attn_transfer per form
    (a) attn_probs, then per segment the dump's columns (converted to fp32, as the payload is) times the payload - the only route to
        all rows there was; (p) attn_probs alone, the part of (a) that no arrangement of its second half removes
    (c) attn_match of the same call: the floor of the walk (the same contraction and exponentials, a running maximum instead of the sums)
  the same layer at R = 68 seeded rows with duplicates
    (t) attn_transfer per form
    (b) attn_rows of the same form, then one matmul per segment over its rows
  the 1024-px top layer at one identity: B 1, H 5, L 16384, N 4, all rows, channels 2 (the dump would be 13.4 GB: not run)

(t), (c) and the attn_rows half of (b) are measured as CALLS_PER_GRAPH calls captured in one graph with events around replays (the
host side of a call would otherwise hide a kernel of tens of microseconds); (a), (p) and (b) as a whole eagerly, events around 4
back-to-back repetitions.  Sides alternate, repeated for SECS seconds (default 1.0), three times; the median of the three.

Every step that touches the GPU is a child process of its own under its own time limit, and the steps are chained: the first one
that fails or runs out of time ends the run (nothing more is started on a device that has just misbehaved).
usage: python tools/gpu_attn_transfer_ab.py [--out FILE]"""
import argparse
import datetime
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

FORMS = ("none", "head_mean")
CALLS_PER_GRAPH = 10
STEPS = [                      # (name, child arguments, time limit in seconds)
    ("top layer, 2 channels", ["--step", "top", "--channels", "2"], 240),
    ("top layer, 4 channels", ["--step", "top", "--channels", "4"], 240),
    ("top layer, 8 channels", ["--step", "top", "--channels", "8"], 240),
    ("1024-px layer, one identity", ["--step", "px1024", "--channels", "2"], 240),
]


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def graph_of(fn):
    import torch
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


def measure(sides, secs):
    import numpy as np
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
    runs = lambda n: "[" + " ".join(f"{x * 1e3:.1f}" for x in meds[n]) + "]"
    return ms, runs


def child(step, channels, secs):
    import numpy as np
    import torch
    from instantrestore_amd import ops
    from instantrestore_amd.attn_maps import coordinate_payload
    B, H, L, N = (8, 5, 4096, 4) if step == "top" else (1, 5, 16384, 4)
    C, S, dt = H * 64, N + 1, torch.bfloat16
    lkv = S * L
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(B, L, C, device="cuda", generator=gen) * 1.2).to(dt)
    k, v = (torch.randn(B, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    rk, rv = (torch.randn(B, N, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    del v, rv
    # channels 0, 1: the (y, x) of every key; further channels: seeded values of the same magnitude
    y = torch.cat([coordinate_payload(L, N, L, True, device="cuda")[0],
                   torch.rand(lkv, channels - 2, device="cuda", generator=gen) * (L ** 0.5)], dim=1).contiguous()
    yseg = y.view(S, L, channels)
    flops = 2.0 * B * H * L * lkv * 64
    dump_bytes = B * H * L * lkv * 2
    out = [f"## B {B} H {H} L {L} N {N} bf16, {channels} channels: {flops / 1e9:.1f} GFLOP of QK^T for all rows, dump {dump_bytes / 1e9:.2f} GB"
           f"   (device: {torch.cuda.get_device_name(0)}, torch {torch.__version__})"]
    graphs, sides = {}, {}
    for f in FORMS:
        graphs["t_" + f] = graph_of(lambda f=f: ops.attn_transfer(q, k, rk, lse, y, None, reduce=f, **kw))
        graphs["c_" + f] = graph_of(lambda f=f: ops.attn_match(q, k, rk, lse, None, reduce=f, **kw))
    if step == "top":
        def dump_route(head_mean):
            p = ops.attn_probs(q, k, rk, lse, **kw).view(B, H, L, S, L)
            sums = torch.stack([p[:, :, :, s].float() @ yseg[s] for s in range(S)], dim=-2)          # (B, H, L, S, channels)
            return sums.mean(1) if head_mean else sums
        # the routes agree: the dump's probabilities carry one bf16 rounding each (2^-9 relative), the sums are at most max|y|
        bound = 2.0 ** -9 * float(y.abs().max()) * 1.05 + 1e-3
        got = ops.attn_transfer(q, k, rk, lse, y, None, reduce="none", **kw)[0]
        d = float((dump_route(False) - got).abs().max())
        assert d <= bound, f"attn_transfer and the dump route differ by {d} (bound {bound})"
        out.append(f"    max |attn_transfer - dump route| over all rows, per head: {d:.3e} (one bf16 rounding per probability: bound {bound:.2e})")
        del got
        torch.cuda.empty_cache()
        sides["a_none"] = lambda: timed(lambda: dump_route(False), 4)
        sides["a_head_mean"] = lambda: timed(lambda: dump_route(True), 4)
        sides["p"] = lambda: timed(lambda: ops.attn_probs(q, k, rk, lse, **kw), 4)
        # R = 68
        rng = np.random.default_rng(0)
        i = rng.integers(0, L, size=(B, 68))
        i[:, 1], i[:, -1] = i[:, 0], i[:, 2]
        idx = torch.from_numpy(i.astype(np.int32)).cuda()

        def rows_route(f):
            r = ops.attn_rows(q, k, rk, lse, idx, reduce=f, **kw)
            r = r.view(*r.shape[:-1], S, L)
            return torch.stack([r[..., s, :].float() @ yseg[s] for s in range(S)], dim=-2)
        for f in FORMS:
            graphs["t68_" + f] = graph_of(lambda f=f: ops.attn_transfer(q, k, rk, lse, y, idx, reduce=f, **kw))
            graphs["r68_" + f] = graph_of(lambda f=f: ops.attn_rows(q, k, rk, lse, idx, reduce=f, **kw))
            sides["b68_" + f] = lambda f=f: timed(lambda: rows_route(f), 4)
        d = float((rows_route("head_mean") - ops.attn_transfer(q, k, rk, lse, y, idx, reduce="head_mean", **kw)[0]).abs().max())
        assert d <= 1e-4 * float(y.abs().max()), f"attn_transfer and attn_rows + matmul differ by {d}"
        out.append(f"    max |attn_transfer - (attn_rows head_mean + matmul)| at R = 68: {d:.3e} (both fp32: bound {1e-4 * float(y.abs().max()):.1e})")
    for name, (g, _keep) in graphs.items():
        sides[name] = lambda g=g: timed(g.replay, 3) / CALLS_PER_GRAPH
    ms, runs = measure(sides, secs)
    for f in FORMS:
        t = ms["t_" + f]
        line = f"(t) attn_transfer {f:9s} all rows: {t * 1e3:9.1f} us  {flops / t / 1e9:7.1f} TFLOP/s of QK^T   this / attn_match {t / ms['c_' + f]:.2f}x"
        if "p" in ms:
            line += f"   dump + matmuls / this {ms['a_' + f] / t:.2f}x   attn_probs alone / this {ms['p'] / t:.2f}x"
        out.append(line + "   " + runs("t_" + f))
    for f in FORMS:
        out.append(f"(c) attn_match    {f:9s} all rows: {ms['c_' + f] * 1e3:9.1f} us   {runs('c_' + f)}")
    if "p" in ms:
        out.append(f"(p) attn_probs alone               : {ms['p'] * 1e3:9.1f} us  {dump_bytes / ms['p'] / 1e9:6.2f} TB/s written   {runs('p')}")
        for f in FORMS:
            out.append(f"(a) attn_probs + matmuls {f:9s} : {ms['a_' + f] * 1e3:9.1f} us   {runs('a_' + f)}")
        for f in FORMS:
            t = ms["t68_" + f]
            out.append(f"(t) attn_transfer {f:9s} R = 68  : {t * 1e3:9.1f} us   attn_rows + matmuls / this {ms['b68_' + f] / t:.2f}x   " + runs("t68_" + f))
            out.append(f"(b) attn_rows + matmuls {f:9s} R = 68: {ms['b68_' + f] * 1e3:9.1f} us (eager; attn_rows alone, captured: {ms['r68_' + f] * 1e3:.1f} us)   "
                       + runs("b68_" + f))
    else:
        out.append(f"(p), (a) not run: the dump would need {dump_bytes / 1e9:.2f} GB per identity")
    print("\n".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=["top", "px1024"], help="(internal) run one measuring step in this process")
    ap.add_argument("--channels", type=int, default=2)
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.0"))
    if args.step is not None:
        child(args.step, args.channels, secs)
        return 0
    lines = [f"# attention-weighted payload sums: attn_transfer vs dump + matmuls, attn_rows + matmuls and attn_match; same box, one process per step, "
             f"alternating, {secs} s x 3, median",
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
