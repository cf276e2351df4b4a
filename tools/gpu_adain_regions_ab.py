"""Same-box A/B of per-region AdaIN (``ir_token_stats_labelled`` / ``ir_adain_apply_labelled``) at cfg 2's three shared layer classes
(bf16, B 8, N 4: 4096 / 1024 / 256 tokens with 5 / 10 / 20 heads), on the strided V views the step hands over (the V third of a
fused q/k/v projection).  The method of profiles/adain_weighted_ab.txt.

(a) statistics, per class the SELF pass over ``(B, 1, L, C)`` and the REFERENCE pass over ``(B, N, L, C)``, with two label maps -
    ``blocks`` (a parsing map: R rectangular cells on the token grid, so a 256-token chunk holds few regions) and ``random`` (every
    chunk holds every region: the worst case of the region loop):
      (rR)  ``ir_token_stats_labelled`` with R = 1 / 4 / 8 / 19 / 32 regions, ONE call
      (i)   ONE ``ir_token_stats_weighted`` call on the same bytes with the 0/1 weights of region 0
      (iiR) R such calls, one per region: the route that exists without the kernel
      (c)   a device copy of the same bytes (``copy_`` into a contiguous tensor)
(b) apply, on the reference V of every class: ``ir_adain_apply_labelled`` (R = 8, both maps) against ``ir_adain_apply`` and against
    a device copy of the same bytes (both read x and write as much)
(c) one shared layer per class through ``SharedAttnProcessor``: with ``adain_regions`` (R = 8, blocks) against the same layer with
    plain (folded) AdaIN, both on this build, and the plain layer on the PARENT commit's library (``--parent-lib``)

Every side of (a) and (b) is a hipGraph of REP back-to-back calls through the C ABI on preallocated buffers (no allocator, no launch
gaps), one replay between two HIP events per sample; a layer of (c) is a hipGraph of LAYER_REP processor calls.  Sides alternate
call by call in a rotating order after a warm-up, for SECS seconds (default 0.6) three times; a side's figure is the median of its
three window means, the three means are printed beside it.

usage: python tools/gpu_adain_regions_ab.py [--parent-lib PATH/libinstantrestore_hip.so] [--out profiles/adain_regions_ab.txt]"""
import argparse
import ctypes as C
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_kv_table_ab import B, CLASSES, N, med, windows  # noqa: E402  (same classes, same windows)

REP, LAYER_REP = 20, 5
REGIONS = (1, 4, 8, 19, 32)


def bind(path):
    """the parent's library beside this build's: every entry point both have, with this build's prototypes (same ABI)"""
    from instantrestore_amd import _lib
    _lib.lib()                                   # torch's HIP runtime first, as _lib.lib() loads it
    h = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return h


def graph_side(fn, rep=REP):
    """fn(stream) issues one call; -> a callable that replays `rep` of them and returns the milliseconds of one"""
    import torch
    from instantrestore_amd import ops
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn(ops._stream())
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(rep):
                fn(ops._stream())
    torch.cuda.current_stream().wait_stream(s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / rep
    return run


def label_map(kind, Bx, M, L, R, gen):
    """int32 (Bx, M, L): `blocks` = R cells of a near-square grid laid over the token grid, `random` = uniform in [0, R)"""
    import math
    import torch
    if kind == "random":
        return torch.randint(0, R, (Bx, M, L), device="cuda", generator=gen, dtype=torch.int32)
    side = int(math.isqrt(L))
    rows = max(1, int(math.isqrt(R)))
    cols = -(-R // rows)
    t = torch.arange(side, device="cuda")
    cell = (t * rows // side)[:, None] * cols + (t * cols // side)[None, :]
    return cell.clamp(max=R - 1).reshape(1, 1, L).expand(Bx, M, L).to(torch.int32).contiguous()


def stats_sides(x, H, kind):
    import torch
    from instantrestore_amd import _lib
    lib = _lib.lib()
    Bx, M, L, _ = x.shape
    gen = torch.Generator(device="cuda").manual_seed(L + M)
    st = (x.stride(0), x.stride(1), x.stride(2), 64)
    nb = max(lib.ir_token_stats_labelled_workspace_bytes(Bx, H, M, L, max(REGIONS)), lib.ir_token_stats_weighted_workspace_bytes(Bx, H, M, L))
    ws = torch.empty(nb // 4, device="cuda")
    mean = torch.empty(Bx, max(REGIONS), M, H, 64, device="cuda")
    std = torch.empty_like(mean)
    mean_w = torch.empty(Bx, M, H, 64, device="cuda")
    std_w = torch.empty_like(mean_w)
    dst = torch.empty(x.shape, dtype=x.dtype, device="cuda")
    keep = [ws, mean, std, mean_w, std_w, dst]
    sides = {"c": graph_side(lambda stream: dst.copy_(x))}
    for R in REGIONS:
        lab = label_map(kind, Bx, M, L, R, gen)
        onehot = [(lab == r).float().contiguous() for r in range(R)]
        keep += [lab] + onehot

        def regions(stream, lab=lab, R=R):
            rc = lib.ir_token_stats_labelled(1, Bx, H, M, L, R, x.data_ptr(), *st, lab.data_ptr(), M * L, L, mean.data_ptr(), std.data_ptr(), None,
                                            ws.data_ptr(), nb, stream)
            assert rc == 0, (rc, lib.ir_last_error_string())

        def weighted(stream, ws_=onehot):
            for w in ws_:
                rc = lib.ir_token_stats_weighted(1, Bx, H, M, L, x.data_ptr(), *st, w.data_ptr(), M * L, L, None, 0,
                                                 mean_w.data_ptr(), std_w.data_ptr(), None, ws.data_ptr(), nb, stream)
                assert rc == 0, (rc, lib.ir_last_error_string())
        sides[f"r{R}"] = graph_side(regions)
        if R == 1:
            continue
        if R == 4:
            sides["i"] = graph_side(lambda stream, w=onehot[0]: weighted(stream, [w]))
        sides[f"ii{R}"] = graph_side(weighted)
    return sides, keep


def apply_sides(x, H):
    import torch
    from instantrestore_amd import _lib
    lib = _lib.lib()
    Bx, M, L, Cc = x.shape
    R = 8
    gen = torch.Generator(device="cuda").manual_seed(L)
    st = (x.stride(0), x.stride(1), x.stride(2), 64)
    y = torch.empty(x.shape, dtype=x.dtype, device="cuda")
    ys = (y.stride(0), y.stride(1), y.stride(2), 64)
    a = torch.rand(Bx, M, R + 1, H, 64, device="cuda", generator=gen) + 0.5
    b = torch.randn(Bx, M, R + 1, H, 64, device="cuda", generator=gen)
    a1, b1 = a[:, :, 0].contiguous(), b[:, :, 0].contiguous()
    labs = {k: label_map(k, Bx, M, L, R, gen) for k in ("blocks", "random")}

    def plain(stream):
        rc = lib.ir_adain_apply(1, Bx, H, M, L, x.data_ptr(), *st, a1.data_ptr(), b1.data_ptr(), y.data_ptr(), *ys, stream)
        assert rc == 0, rc

    def regions(lab):
        def fn(stream):
            rc = lib.ir_adain_apply_labelled(1, Bx, H, M, L, R, x.data_ptr(), *st, lab.data_ptr(), M * L, L, a.data_ptr(), b.data_ptr(),
                                            y.data_ptr(), *ys, stream)
            assert rc == 0, (rc, lib.ir_last_error_string())
        return fn
    sides = {"plain": graph_side(plain), "blocks": graph_side(regions(labs["blocks"])), "random": graph_side(regions(labs["random"])),
             "copy": graph_side(lambda stream: y.copy_(x))}
    return sides, [y, a, b, a1, b1, labs]


def layer_sides(L, H, parent):
    import torch
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd import _lib
    from instantrestore_amd.attention import Attention
    dt, R = torch.bfloat16, 8
    gen = torch.Generator(device="cuda").manual_seed(L + H)
    torch.manual_seed(L)
    attn = Attention(query_dim=H * 64, heads=H, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=True)).eval().cuda().to(dt)
    hidden = torch.randn(B, L, H * 64, device="cuda", generator=gen).to(dt)
    rk = torch.randn(B, N, L, H * 64, device="cuda", generator=gen).to(dt)
    rv = (torch.randn(B, N, L, H * 64, device="cuda", generator=gen) * 1.2 + 0.3).to(dt)
    ql, rl = label_map("blocks", B, 1, L, R, gen)[:, 0].contiguous(), label_map("blocks", B, N, L, R, gen)
    refs = {"ref_keys": [rk], "ref_values": [rv]}

    def call(**kw):
        def fn(stream):
            with torch.no_grad(), torch.autocast("cuda", dtype=dt):
                return attn(hidden, **refs, **kw)
        return fn
    sides = {"plain": graph_side(call(), LAYER_REP), "regions": graph_side(call(adain_regions=(ql, rl), adain_n_regions=R), LAYER_REP)}
    if parent is not None:
        mine, _lib._lib = _lib._lib, parent         # the plain layer captured on the parent's kernels
        try:
            sides["parent"] = graph_side(call(), LAYER_REP)
        finally:
            _lib._lib = mine
    return sides, [attn, hidden, rk, rv, ql, rl]


def row(x, mb=None):
    bw = f"  {mb / (med(x) * 1e3):5.2f} TB/s read" if mb is not None else ""
    return f"{med(x) * 1e3:9.2f} us{bw}  [{' '.join(f'{v * 1e3:.2f}' for v in x)}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libinstantrestore_hip.so built from the parent commit; without it the parent side of (c) is skipped")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    secs = float(os.environ.get("SECS", "0.6"))
    import torch
    from instantrestore_amd import _lib
    parent = bind(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    lines = [f"# per-region AdaIN, cfg 2 (bf16, B {B}, N {N}), same box, same process, same tensors; hipGraphs of {REP} calls ({LAYER_REP} layer "
             f"calls in (c)), sides alternating replay by replay, {secs} s x 3, median of the window means [the three window means]",
             f"# device: {torch.cuda.get_device_name(0)}  date: {datetime.date.today().isoformat()}  torch {torch.__version__}  "
             f"{_lib.lib().ir_build_info().decode()}" + (f"  parent: {parent.ir_build_info().decode()}" if parent is not None else "")]
    for L, H in CLASSES:
        Cc = H * 64
        gen = torch.Generator(device="cuda").manual_seed(L + H)
        qkv_self = (torch.randn(B, L, 3 * Cc, device="cuda", generator=gen) + 0.3).to(torch.bfloat16)
        qkv_ref = (torch.randn(B * N, L, 3 * Cc, device="cuda", generator=gen) * 1.2 + 0.3).to(torch.bfloat16)
        x_self, x_ref = qkv_self[..., 2 * Cc:].unsqueeze(1), qkv_ref[..., 2 * Cc:].unflatten(0, (B, N))
        for what, x in (("self pass (B, 1, L, C)", x_self), ("reference pass (B, N, L, C)", x_ref)):
            mb = x.numel() * 2 / 1e6
            for kind in ("blocks", "random"):
                sides, keep = stats_sides(x, H, kind)
                res = windows(sides, secs)
                lines.append(f"## (a) L {L} H {H}: {what}, {mb:.1f} MB, labels: {kind}")
                lines.append(f"(c)    device copy of the same bytes              : {row(res['c'], mb)}")
                lines.append(f"(i)    ONE weighted call, 0/1 weights of region 0 : {row(res['i'], mb)}")
                for R in REGIONS:
                    one = med(res[f"r{R}"])
                    txt = f"(r{R})".ljust(6) + f" token_stats_regions, R = {R:2d}, one call       : {row(res[f'r{R}'], mb)}   r/i {one / med(res['i']):.2f}"
                    if R > 1:
                        many = med(res[f"ii{R}"])
                        txt += f"   | (ii{R}) {R} weighted calls: {row(res[f'ii{R}'])}   r/ii {one / many:.3f}" + \
                               (f"  {'FASTER' if one < many else 'NOT FASTER'}" if R >= 4 else "")
                    lines.append(txt)
                del sides, keep
        mb = x_ref.numel() * 2 / 1e6
        sides, keep = apply_sides(x_ref, H)
        res = windows(sides, secs)
        lines.append(f"## (b) L {L} H {H}: apply over the reference V (B, N, L, C), {mb:.1f} MB read and as much written")
        for n, name in (("plain", "ir_adain_apply"), ("blocks", "ir_adain_apply_labelled, R = 8, blocks"), ("random", "ir_adain_apply_labelled, R = 8, random"),
                        ("copy", "device copy (read + written)")):
            lines.append(f"{name:40s}: {row(res[n], mb)}")
        spread = max(max(v) - min(v) for v in res.values())
        lines.append(f"regions(blocks) - plain {(med(res['blocks']) - med(res['plain'])) * 1e3:+.2f} us, regions(random) - plain "
                     f"{(med(res['random']) - med(res['plain'])) * 1e3:+.2f} us, largest spread of a side {spread * 1e3:.2f} us")
        del sides, keep
        sides, keep = layer_sides(L, H, parent)
        res = windows(sides, secs)
        lines.append(f"## (c) L {L} H {H}: one shared layer through SharedAttnProcessor (q/k/v GEMMs, AdaIN, attention, out projection)")
        lines.append(f"plain (folded) AdaIN, this build         : {row(res['plain'])}")
        lines.append(f"adain_regions, R = 8, blocks, this build : {row(res['regions'])}   regions - plain {(med(res['regions']) - med(res['plain'])) * 1e3:+.2f} us "
                     f"({med(res['regions']) / med(res['plain']):.3f}x)")
        if "parent" in res:
            spread, excess = max(res["parent"]) - min(res["parent"]), abs(med(res["plain"]) - med(res["parent"]))
            lines.append(f"plain (folded) AdaIN, the parent's library: {row(res['parent'])}   |plain - parent| {excess * 1e3:.2f} us, spread of the parent "
                         f"{spread * 1e3:.2f} us: {'inside' if excess <= spread else 'OUTSIDE'}   plain/parent {med(res['plain']) / med(res['parent']):.4f}")
        del sides, keep, qkv_self, qkv_ref, x_self, x_ref
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
