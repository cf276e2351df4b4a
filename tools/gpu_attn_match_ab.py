"""Same-box, one-process A/B of the best-match read-out (``ops.attn_match``) against the only route there was before it - the whole
dump followed by a maximum per segment (``ops.attn_probs(...)`` then ``torch.max`` over each segment's columns), where the dump
fits - and against ``ops.attn_probs`` alone and ``ops.attn_segment_mass`` on the same shapes.

  cfg 2's three shared layer classes: bf16, B 8, N 4, self included, (H, L) = (20, 256), (10, 1024), (5, 4096); all rows, both forms
  cfg 2's top layer with R = 68 seeded rows with duplicates
  the 1024-px top layer at one identity: B 1, H 5, L 16384, all rows (the dump would be 13.4 GB: not run)

  (m) attn_match per form, CALLS_PER_GRAPH calls captured in one graph, events around replays (the host side of a call - argument
      checks, the allocations - would otherwise hide a kernel of tens of microseconds)
  (s) attn_segment_mass, the same way
  (p) attn_probs alone and (a) attn_probs + max per segment, eager, events around 4 back-to-back repetitions (where the dump fits)
  (c) a device-to-device copy of 256 MB, the same way as (m): the copy rate the box gives during this run

Sides alternate, repeated for SECS seconds (default 1.0), three times; the median of the three.
usage: python tools/gpu_attn_match_ab.py [--out FILE]"""
import argparse
import datetime
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantrestore_amd import ops  # noqa: E402

FORMS = ("none", "head_mean")
CALLS_PER_GRAPH = 10
COPY_BYTES = 256 << 20


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


def layer(B, H, L, N, R, secs, with_dump, lines):
    C = H * 64
    dt = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn(B, L, C, device="cuda", generator=gen) * 1.2).to(dt)
    k, v = (torch.randn(B, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    rk, rv = (torch.randn(B, N, L, C, device="cuda", generator=gen).to(dt) for _ in range(2))
    _, lse = ops.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True)
    del v, rv
    S = N + 1
    lkv = S * L
    if R is None:
        idx, nrows = None, L
    else:
        rng = np.random.default_rng(0)
        i = rng.integers(0, L, size=(B, R))
        i[:, 1], i[:, -1] = i[:, 0], i[:, 2]
        idx, nrows = torch.from_numpy(i.astype(np.int32)).cuda(), R
    kbytes = B * H * lkv * 64 * 2
    groups = (nrows + 95) // 96
    flops = 2.0 * B * H * nrows * lkv * 64
    dump_bytes = B * H * L * lkv * 2
    lines.append(f"## B {B} H {H} L {L} N {N} rows {'all' if R is None else R} bf16: K {kbytes / 1e6:.1f} MB read by {groups} row group(s), "
                 f"{flops / 1e9:.1f} GFLOP of QK^T, dump {dump_bytes / 1e9:.2f} GB")
    kw = dict(heads=H, scale=0.125, include_self=True)
    sides, graphs = {}, {}
    full = R is None
    if with_dump and full:
        def dump_max():
            p = ops.attn_probs(q, k, rk, lse, **kw)
            m = p.view(B, H, L, S, L).max(-1)
            return m.indices, m.values
        # the two routes agree (the dump's maximum is the rounded prob; its argmax attains it)
        di, dv = dump_max()
        mi, mv = ops.attn_match(q, k, rk, lse, None, reduce="none", **kw)
        assert torch.equal(mv.to(dt), dv), "per-head prob differs from the dump's maximum"
        p = ops.attn_probs(q, k, rk, lse, **kw).view(B, H, L, S, L)
        assert torch.equal(p.gather(-1, mi.long().unsqueeze(-1))[..., 0], dv), "per-head index does not attain the dump's maximum"
        del di, dv, mi, mv, p
        sides["a"] = lambda: timed(dump_max, 4)
        sides["p"] = lambda: timed(lambda: ops.attn_probs(q, k, rk, lse, **kw), 4)
    for f in FORMS:
        graphs["m_" + f] = graph_of(lambda f=f: ops.attn_match(q, k, rk, lse, idx, reduce=f, **kw))
    if full:
        graphs["s"] = graph_of(lambda: ops.attn_segment_mass(q, k, rk, lse, **kw))
    src = torch.empty(COPY_BYTES // 2, dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    graphs["c"] = graph_of(lambda: dst.copy_(src))
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
    runs = lambda n: "[" + " ".join(f"{x * 1e3:.1f}" for x in meds[n]) + "]"
    for f in FORMS:
        t = ms["m_" + f]
        line = f"(m) attn_match {f:9s}: {t * 1e3:9.1f} us  {flops / t / 1e9:7.1f} TFLOP/s of QK^T  {groups * kbytes / t / 1e9:6.2f} TB/s of K over the row groups"
        if "p" in ms:
            line += f"   attn_probs alone / this {ms['p'] / t:.2f}x   dump + max / this {ms['a'] / t:.2f}x"
        if "s" in ms:
            line += f"   this / attn_segment_mass {t / ms['s']:.2f}x"
        lines.append(line + "   " + runs("m_" + f))
    lines.append(f"    head_mean / none: {ms['m_head_mean'] / ms['m_none']:.2f}x")
    if "s" in ms:
        lines.append(f"(s) attn_segment_mass   : {ms['s'] * 1e3:9.1f} us   {runs('s')}")
    if "p" in ms:
        lines.append(f"(p) attn_probs alone    : {ms['p'] * 1e3:9.1f} us  {dump_bytes / ms['p'] / 1e9:6.2f} TB/s written   {runs('p')}")
        lines.append(f"(a) attn_probs + max    : {ms['a'] * 1e3:9.1f} us   {runs('a')}")
    elif full:
        lines.append(f"(p), (a) not run: the dump would need {dump_bytes / 1e9:.2f} GB per identity")
    lines.append(f"(c) copy of {COPY_BYTES >> 20} MB (read + written): {ms['c'] * 1e3:9.1f} us  {COPY_BYTES / ms['c'] / 1e9:6.2f} TB/s   {runs('c')}")
    del graphs, sides
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.0"))
    lines = [f"# best match per segment: attn_match vs dump + max, attn_probs alone and attn_segment_mass; same box, one process, alternating, {secs} s x 3, median",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}"]
    layer(8, 20, 256, 4, None, secs, True, lines)
    layer(8, 10, 1024, 4, None, secs, True, lines)
    layer(8, 5, 4096, 4, None, secs, True, lines)
    layer(8, 5, 4096, 4, 68, secs, False, lines)
    layer(1, 5, 16384, 4, None, secs, False, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
