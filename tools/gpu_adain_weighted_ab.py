"""Same-box A/B of the mask-aware AdaIN statistics (``ir_token_stats_weighted``) at cfg 2's three shared layer classes (bf16, B 8,
N 4: 4096 / 1024 / 256 tokens with 5 / 10 / 20 heads), on the strided V views the step hands over (the V third of a fused q/k/v
projection).  Two passes per class - the SELF pass over ``(B, 1, L, C)`` and the REFERENCE pass over ``(B, N, L, C)`` - and per pass:

  (a) ``ir_token_stats``, this build                         (p) the same on the PARENT commit's library (``--parent-lib``) - the yardstick
  (n) ``ir_token_stats_weighted``, weights NULL, lens NULL   (w) ... with a 0/1 mask that keeps half the tokens
  (s) ... with soft weights in [0, 1]                        (l) ... with counts in [L / 2, L]
  (c) a device copy of the same bytes (``copy_`` into a contiguous tensor: the read plus as much again written)
  (k) ``ir_adain_stats_cached``, this build (self pass only) (q) the same on the parent's library

What to read off: (a) against (p) and (k) against (q) - the existing calls are the code they were (their difference has to sit
inside the spread of the yardstick's windows); (n)/(a) - what carrying W and W2 costs; (w)/(a), (s)/(a), (l)/(a) - what the weights
row and the counts cost (a mask or a count also removes work: dropped rows skip the arithmetic, not the load); (a)/(c) - where the
pass sits against the memory system.

Every side is a hipGraph of REP back-to-back calls through the C ABI on preallocated buffers (no allocator, no launch gaps), one
replay between two HIP events per sample.  Both libraries run in this process on the same tensors.  Sides alternate call by call
in a rotating order after a warm-up, for SECS seconds (default 1.0) three times; a side's figure is the median of its three window
means, the three means are printed beside it.

usage: python tools/gpu_adain_weighted_ab.py --parent-lib PATH/libinstantrestore_hip.so [--out profiles/adain_weighted_ab.txt]"""
import argparse
import ctypes as C
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_kv_table_ab import B, CLASSES, N, med, windows  # noqa: E402  (same classes, same windows)

REP = 20


def bind(path):
    """the parent's library beside this build's: the three entry points both have, with this build's prototypes (same ABI)"""
    from instantrestore_amd import _lib
    _lib.lib()                                   # torch's HIP runtime first, as _lib.lib() loads it
    h = C.CDLL(path)
    for name in ("ir_adain_stats_workspace_bytes", "ir_token_stats", "ir_adain_stats_cached", "ir_build_info"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return h


def graph_side(fn):
    """fn(stream) issues one call; -> a callable that replays REP of them and returns the milliseconds of one"""
    import torch
    from instantrestore_amd import ops
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn(ops._stream())
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REP):
                fn(ops._stream())
    torch.cuda.current_stream().wait_stream(s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / REP
    return run


def pass_sides(x, H, parent, cached):
    """x: (B, M, L, C) bf16 strided view -> {side: callable}"""
    import torch
    from instantrestore_amd import _lib
    lib = _lib.lib()
    Bx, M, L, _ = x.shape
    gen = torch.Generator(device="cuda").manual_seed(L + M)
    mean = torch.empty(Bx, M, H, 64, device="cuda")
    std = torch.empty_like(mean)
    nb = max(lib.ir_adain_stats_workspace_bytes(Bx, H, L, M - 1, L), lib.ir_token_stats_weighted_workspace_bytes(Bx, H, M, L))
    ws = torch.empty(nb // 4, device="cuda")
    mask = (torch.rand(Bx, M, L, device="cuda", generator=gen) < 0.5).float()
    soft = torch.rand(Bx, M, L, device="cuda", generator=gen)
    lens = torch.randint(L // 2, L + 1, (Bx, M), device="cuda", generator=gen, dtype=torch.int32)
    dst = torch.empty(x.shape, dtype=x.dtype, device="cuda")
    keep = [mean, std, ws, mask, soft, lens, dst]
    st = (x.stride(0), x.stride(1), x.stride(2), 64)

    def plain(h):
        def fn(stream):
            rc = h.ir_token_stats(1, Bx, H, M, L, x.data_ptr(), *st, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), nb, stream)
            assert rc == 0, rc
        return fn

    def weighted(w, ln):
        def fn(stream):
            rc = lib.ir_token_stats_weighted(1, Bx, H, M, L, x.data_ptr(), *st, None if w is None else w.data_ptr(), M * L, L,
                                             None if ln is None else ln.data_ptr(), M, mean.data_ptr(), std.data_ptr(), None,
                                             ws.data_ptr(), nb, stream)
            assert rc == 0, (rc, lib.ir_last_error_string())
        return fn

    sides = {"a": graph_side(plain(lib)), "n": graph_side(weighted(None, None)), "w": graph_side(weighted(mask, None)),
             "s": graph_side(weighted(soft, None)), "l": graph_side(weighted(None, lens)), "c": graph_side(lambda stream: dst.copy_(x))}
    if parent is not None:
        sides["p"] = graph_side(plain(parent))
    if cached:
        v = x[:, 0]
        cm = torch.randn(Bx, N, H, 64, device="cuda", generator=gen)
        cs = torch.rand(Bx, N, H, 64, device="cuda", generator=gen) + 0.5
        a = torch.empty(Bx, N, H, 64, device="cuda")
        b = torch.empty_like(a)
        keep += [cm, cs, a, b]

        def cached_call(h):
            def fn(stream):
                rc = h.ir_adain_stats_cached(1, Bx, H, L, N, v.data_ptr(), v.stride(0), v.stride(1), 64, cm.data_ptr(), cs.data_ptr(), 1e-5,
                                             a.data_ptr(), b.data_ptr(), ws.data_ptr(), nb, stream)
                assert rc == 0, rc
            return fn
        sides["k"] = graph_side(cached_call(lib))
        if parent is not None:
            sides["q"] = graph_side(cached_call(parent))
    return sides, keep


NAMES = (("a", "ir_token_stats, this build"), ("p", "ir_token_stats, the parent's library"), ("n", "weighted: weights NULL, lens NULL"),
         ("w", "weighted: 0/1 mask, half the tokens kept"), ("s", "weighted: soft weights in [0, 1]"), ("l", "weighted: counts in [L / 2, L]"),
         ("c", "device copy of the same bytes"), ("k", "ir_adain_stats_cached, this build"), ("q", "ir_adain_stats_cached, the parent's library"))


def fmt(x, mb):
    return f"{med(x) * 1e3:8.2f} us  {mb / (med(x) * 1e3):5.2f} TB/s read  [{' '.join(f'{v * 1e3:.2f}' for v in x)}]"


def inside(res, new, yard):
    spread, excess = max(res[yard]) - min(res[yard]), abs(med(res[new]) - med(res[yard]))
    return (f"({new}) vs ({yard}): |{new} - {yard}| {excess * 1e3:.2f} us, spread of ({yard}) {spread * 1e3:.2f} us: "
            f"{'inside' if excess <= spread else 'OUTSIDE'}   {new}/{yard} {med(res[new]) / med(res[yard]):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libinstantrestore_hip.so built from the parent commit; without it (p) and (q) are skipped")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "1.0"))
    import torch
    from instantrestore_amd import _lib
    parent = bind(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    lines = [f"# mask-aware AdaIN statistics, cfg 2 (bf16, B {B}, N {N}), same box, same process, same tensors; hipGraphs of {REP} calls, sides "
             f"alternating replay by replay, {secs} s x 3, median of the window means [the three window means]",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}  "
             f"{_lib.lib().ir_build_info().decode()}" + (f"  parent: {parent.ir_build_info().decode()}" if parent is not None else "")]
    for L, H in CLASSES:
        Cc = H * 64
        gen = torch.Generator(device="cuda").manual_seed(L + H)
        qkv_self = (torch.randn(B, L, 3 * Cc, device="cuda", generator=gen) + 0.3).to(torch.bfloat16)
        qkv_ref = (torch.randn(B * N, L, 3 * Cc, device="cuda", generator=gen) * 1.2 + 0.3).to(torch.bfloat16)
        for what, x, cached in (("self pass (B, 1, L, C)", qkv_self[..., 2 * Cc:].unsqueeze(1), True),
                                ("reference pass (B, N, L, C)", qkv_ref[..., 2 * Cc:].unflatten(0, (B, N)), False)):
            mb = x.numel() * 2 / 1e6
            sides, keep = pass_sides(x, H, parent, cached)
            res = windows(sides, secs)
            lines.append(f"## L {L} H {H}: {what}, {mb:.1f} MB")
            for n, name in NAMES:
                if n in res:
                    lines.append(f"({n}) {name:45s}: {fmt(res[n], mb)}")
            if "p" in res:
                lines.append(inside(res, "a", "p"))
            if "q" in res:
                lines.append(inside(res, "k", "q"))
            a = med(res["a"])
            lines.append(f"(n)/(a) {med(res['n']) / a:.4f}   (w)/(a) {med(res['w']) / a:.4f}   (s)/(a) {med(res['s']) / a:.4f}   (l)/(a) {med(res['l']) / a:.4f}   "
                         f"(a)/(c) {a / med(res['c']):.4f}   (s) - (a) {(med(res['s']) - a) * 1e3:.2f} us, largest spread of a side "
                         f"{max(max(v) - min(v) for v in res.values()) * 1e3:.2f} us")
            del sides, keep
        del qkv_self, qkv_ref
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
