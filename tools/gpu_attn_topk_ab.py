"""Same-box A/B of the top-k read-out (``ops.attn_topk``) against the routes there were before it, bf16, N 4, self included:

  cfg 2's three shared classes at B 8 - H 20 L 256, H 10 L 1024, H 5 L 4096 - and the 1024-px top layer at one identity (B 1, H 5,
  L 16384: the dump would be 13.4 GB and is not run), all rows and R = 68 seeded rows with duplicates
    (d) attn_topk at k = 2, 4, 8, both forms
    (a) attn_probs, then torch.topk over every segment of the dump (per head; the head mean - the dump's mean over the heads in
        fp32 first - at k = 4): the only route to all rows there was
    (p) attn_probs alone, the part of (a) that no arrangement of its second half removes
    (c) attn_match of the same call: the floor of the walk (the same contraction and exponentials, one running pair instead of
        the sorted list)
    (b) at R = 68: attn_rows of the same form, then torch.topk over every segment of its rows (k = 4)

Before anything is timed, rank 0 of every (d) is held to (c) with torch.equal.

(d), (c) and the attn_rows half of (b) are measured as CALLS_PER_GRAPH calls captured in one graph with events around replays (the
host side of a call would otherwise hide a kernel of tens of microseconds); (a), (p) and (b) as a whole eagerly, events around
back-to-back repetitions.  Sides alternate, repeated for SECS seconds (default 1.0), three times; the median of the three.

Every step that touches the GPU is a child process of its own under its own time limit, and the steps are chained: the first one
that fails or runs out of time ends the run (nothing more is started on a device that has just misbehaved).
usage: python tools/gpu_attn_topk_ab.py [--out FILE]"""
import argparse
import datetime
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from gpu_attn_transfer_ab import CALLS_PER_GRAPH, graph_of, measure, timed  # noqa: E402  (the machinery of the payload read-out's A/B)

FORMS = ("none", "head_mean")
KS = (2, 4, 8)
CLASSES = {"L256": (8, 20, 256), "L1024": (8, 10, 1024), "L4096": (8, 5, 4096), "px1024": (1, 5, 16384)}      # B, H, L
STEPS = [(f"{name}: B {b} H {h} L {l}", ["--step", name], 240) for name, (b, h, l) in CLASSES.items()]        # (name, child arguments, time limit in seconds)


def child(step, secs):
    import numpy as np
    import torch
    from instantrestore_amd import ops
    B, H, L = CLASSES[step]
    N = 4
    C, S, dt = H * 64, N + 1, torch.bfloat16
    lkv = S * L
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(B, L, C, device="cuda", generator=gen) * 1.2).to(dt)
    k, v = (torch.randn(B, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    rk, rv = (torch.randn(B, N, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    del v, rv
    flops = 2.0 * B * H * L * lkv * 64
    dump_bytes = B * H * L * lkv * 2
    with_dump = step != "px1024"
    out = [f"## B {B} H {H} L {L} N {N} bf16: {flops / 1e9:.1f} GFLOP of QK^T for all rows, dump {dump_bytes / 1e9:.2f} GB"
           f"   (device: {torch.cuda.get_device_name(0)}, torch {torch.__version__})"]
    rng = np.random.default_rng(0)
    i = rng.integers(0, L, size=(B, 68))
    i[:, 1], i[:, -1] = i[:, 0], i[:, 2]
    idx = torch.from_numpy(i.astype(np.int32)).cuda()

    # rank 0 of (d) IS (c): before anything is timed
    for rows in (None, idx):
        for f in FORMS:
            mi, mp = ops.attn_match(q, k, rk, lse, rows, reduce=f, **kw)
            for kk in KS:
                ti, tp = ops.attn_topk(q, k, rk, lse, rows, k=kk, reduce=f, **kw)
                assert torch.equal(ti[..., 0], mi) and torch.equal(tp[..., 0], mp), f"rank 0 of attn_topk is not attn_match ({f}, k = {kk})"
    out.append("    rank 0 of attn_topk == attn_match (torch.equal): both forms, k = 2, 4, 8, all rows and R = 68")

    graphs, sides = {}, {}
    for f in FORMS:
        graphs["c_" + f] = graph_of(lambda f=f: ops.attn_match(q, k, rk, lse, None, reduce=f, **kw))
        graphs["c68_" + f] = graph_of(lambda f=f: ops.attn_match(q, k, rk, lse, idx, reduce=f, **kw))
        graphs["r68_" + f] = graph_of(lambda f=f: ops.attn_rows(q, k, rk, lse, idx, reduce=f, **kw))
        for kk in KS:
            graphs[f"d_{f}_{kk}"] = graph_of(lambda f=f, kk=kk: ops.attn_topk(q, k, rk, lse, None, k=kk, reduce=f, **kw))
            graphs[f"d68_{f}_{kk}"] = graph_of(lambda f=f, kk=kk: ops.attn_topk(q, k, rk, lse, idx, k=kk, reduce=f, **kw))

    def rows_route(f, kk):
        r = ops.attn_rows(q, k, rk, lse, idx, reduce=f, **kw)
        return torch.topk(r.view(*r.shape[:-1], S, L), kk, dim=-1)
    for f in FORMS:
        sides["b68_" + f] = lambda f=f: timed(lambda: rows_route(f, 4), 4)
    if with_dump:
        def dump_route(kk, head_mean):
            p = ops.attn_probs(q, k, rk, lse, **kw)
            if head_mean:
                p = p.mean(dim=1, dtype=torch.float32)
            return torch.topk(p.view(*p.shape[:-1], S, L), kk, dim=-1)
        # the routes agree: the dump's values carry one bf16 rounding each, so its k largest are the rounded k largest
        got = ops.attn_topk(q, k, rk, lse, None, k=4, reduce="none", **kw)[1]
        want = dump_route(4, False).values
        assert torch.equal(got.to(dt), want), "attn_topk and the dump route differ"
        out.append("    attn_topk prob rounded to bf16 == torch.topk of the dump (torch.equal): per head, k = 4, all rows")
        del got, want
        torch.cuda.empty_cache()
        reps = 4 if L < 4096 else 2
        for kk in KS:
            sides[f"a_none_{kk}"] = lambda kk=kk: timed(lambda: dump_route(kk, False), reps)
        sides["a_head_mean_4"] = lambda: timed(lambda: dump_route(4, True), reps)
        sides["p"] = lambda: timed(lambda: ops.attn_probs(q, k, rk, lse, **kw), reps)
    for name, (g, _keep) in graphs.items():
        sides[name] = lambda g=g: timed(g.replay, 3) / CALLS_PER_GRAPH
    ms, runs = measure(sides, secs)
    for f in FORMS:
        for kk in KS:
            t = ms[f"d_{f}_{kk}"]
            line = f"(d) attn_topk k={kk} {f:9s} all rows: {t * 1e3:9.1f} us  {flops / t / 1e9:7.1f} TFLOP/s of QK^T   this / attn_match {t / ms['c_' + f]:.2f}x"
            a = ms.get(f"a_{f}_{kk}")
            if a is not None:
                line += f"   dump + topk / this {a / t:.2f}x   attn_probs alone / this {ms['p'] / t:.2f}x"
            out.append(line + "   " + runs(f"d_{f}_{kk}"))
    for f in FORMS:
        out.append(f"(c) attn_match     {f:9s} all rows: {ms['c_' + f] * 1e3:9.1f} us   {runs('c_' + f)}")
    if with_dump:
        out.append(f"(p) attn_probs alone                 : {ms['p'] * 1e3:9.1f} us  {dump_bytes / ms['p'] / 1e9:6.2f} TB/s written   {runs('p')}")
        for kk in KS:
            out.append(f"(a) attn_probs + topk k={kk} none      : {ms[f'a_none_{kk}'] * 1e3:9.1f} us   {runs(f'a_none_{kk}')}")
        out.append(f"(a) attn_probs + mean + topk k=4 head_mean: {ms['a_head_mean_4'] * 1e3:9.1f} us   {runs('a_head_mean_4')}")
    else:
        out.append(f"(p), (a) not run: the dump would need {dump_bytes / 1e9:.2f} GB per identity")
    for f in FORMS:
        for kk in KS:
            t = ms[f"d68_{f}_{kk}"]
            line = f"(d) attn_topk k={kk} {f:9s} R = 68  : {t * 1e3:9.1f} us   this / attn_match {t / ms['c68_' + f]:.2f}x"
            if kk == 4:
                line += f"   attn_rows + topk / this {ms['b68_' + f] / t:.2f}x"
            out.append(line + "   " + runs(f"d68_{f}_{kk}"))
        out.append(f"(c) attn_match     {f:9s} R = 68  : {ms['c68_' + f] * 1e3:9.1f} us   {runs('c68_' + f)}")
        out.append(f"(b) attn_rows + topk k=4 {f:9s} R = 68: {ms['b68_' + f] * 1e3:9.1f} us (eager; attn_rows alone, captured: {ms['r68_' + f] * 1e3:.1f} us)   "
                   + runs("b68_" + f))
    print("\n".join(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(CLASSES), help="(internal) run one measuring step in this process")
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.0"))
    if args.step is not None:
        child(args.step, secs)
        return 0
    lines = [f"# the k best keys per segment: attn_topk vs dump + torch.topk, attn_probs alone, attn_match and attn_rows + torch.topk; same box, one process "
             f"per step, alternating, {secs} s x 3, median",
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
