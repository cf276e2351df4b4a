"""Same-box, alternating A/B of the batch-invariant mode (ABI v10) against the default dispatch.

Usage: gpu_batch_invariant_ab.py [cfg ...]   (default: cfg2 cfg1gpu)

For each config: the nine-layer attention step as ``bench.build_workload`` builds it (K/V capture -> shared attention, one stream,
eager, bf16 / fp16 autocast over fp32 activations), A = default, B = every processor's ``batch_invariant`` set
(``attn_processors.set_batch_invariant``), ROUNDS interleaved rounds of STEPS timed steps each after a warm-up; then, per layer
class and in both modes, the calls the step is made of: the shared attention launch, the K/V-capture layer's self-attention over
B*N reference sets, and the four projection GEMMs (with the per-call scratch the mode allocates), summed into what each part adds
to the step.  Prints medians and ratios."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from instantrestore_amd import ops  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "8"))
STEPS = int(os.environ.get("STEPS", "10"))
LOG2E = 1.4426950408889634


def set_mode(layers, on):
    for ly in layers:
        for m in (ly["kv_attn"], ly["main_attn"]):
            m.processor.batch_invariant = on


def time_steps(layers, B, N, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        e0.record()
        for _ in range(steps):
            bench.hot_path_step(layers, B, N)
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def _median_pair(fa, fb, reps=5):
    """alternating medians of two timed callables (ms)"""
    a, b = [], []
    for _ in range(reps):
        a.append(fa())
        b.append(fb())
    return statistics.median(a), statistics.median(b)


def _time_calls(fn, iters=20):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def class_times(layers, B, N, dtype, iters=20):
    """per layer class (first layer of the class; each class has three layers in the step), both modes, ms per call:
    the shared attention launch (pre-scaled Q, AdaIN fold), the K/V-capture layer's self-attention over B*N reference token sets
    (pre-scaled Q, as AttnProcessor runs it), and the four projections of the step - capture q/k/v (fp32 activations, pre-scaled q
    third, statistics tail of the V third), capture out (bias), shared q/k/v (same form), shared out (bias) - plus the per-call
    scratch the mode allocates for the two attention calls"""
    g = torch.Generator().manual_seed(5)
    rows = []
    seen = set()
    with torch.no_grad():
        for ly in layers:
            L, C, H = ly["L"], ly["C"], ly["H"]
            if L in seen:
                continue
            seen.add(L)
            r = dict(L=L, H=H)
            q = (torch.randn(B, L, C, generator=g) * (0.125 * LOG2E)).to("cuda", dtype)
            ks, vs = torch.randn(B, L, C, generator=g).to("cuda", dtype), torch.randn(B, L, C, generator=g).to("cuda", dtype)
            rk, rv = torch.randn(B, N, L, C, generator=g).to("cuda", dtype), torch.randn(B, N, L, C, generator=g).to("cuda", dtype)
            aff = ops.adain_stats(vs, rv, heads=H)
            kw = dict(heads=H, scale=0.125, include_self=True, adain=aff, q_prescaled=True, iters=iters)
            r["shared"] = _median_pair(lambda: ops.time_shared_attention(q, ks, vs, rk, rv, **kw),
                                       lambda: ops.time_shared_attention(q, ks, vs, rk, rv, batch_invariant=True, **kw))
            r["shared_names"] = (ops.shared_attention_kernel_name(q, ks, vs, rk, rv, heads=H, scale=0.125, adain=aff, q_prescaled=True),
                                 ops.shared_attention_kernel_name(q, ks, vs, rk, rv, heads=H, scale=0.125, adain=aff, q_prescaled=True,
                                                                  batch_invariant=True))
            r["shared_ws"] = ops.shared_attention_plan(B, L, H, len_self=L, n_refs=N, len_ref=L, dtype=dtype, adain=True,
                                                       q_prescaled=True)
            del q, ks, vs, rk, rv, aff
            qc = (torch.randn(B * N, L, C, generator=g) * (0.125 * LOG2E)).to("cuda", dtype)
            kc, vc = torch.randn(B * N, L, C, generator=g).to("cuda", dtype), torch.randn(B * N, L, C, generator=g).to("cuda", dtype)
            kwc = dict(heads=H, scale=0.125, include_self=True, q_prescaled=True, iters=iters)
            r["capture"] = _median_pair(lambda: ops.time_shared_attention(qc, kc, vc, **kwc),
                                        lambda: ops.time_shared_attention(qc, kc, vc, batch_invariant=True, **kwc))
            r["capture_ws"] = ops.shared_attention_plan(B * N, L, H, len_self=L, dtype=dtype, q_prescaled=True)
            del qc, kc, vc
            w3 = (torch.randn(3 * C, C, generator=g) / C ** 0.5).to("cuda", dtype)
            w1 = (torch.randn(C, C, generator=g) / C ** 0.5).to("cuda", dtype)
            b1 = torch.randn(C, generator=g).to("cuda", dtype)
            gemms = {}
            for tag, rows_ in (("capture", B * N), ("shared", B)):
                x32 = torch.randn(rows_, L, C, generator=g).to("cuda")
                x16 = x32.to(dtype)
                qkv = dict(scale_cols=C, col_scale=0.125 * LOG2E, stats=(2 * C, C))
                gemms[f"{tag} qkv M={rows_ * L} N={3 * C} K={C}"] = _median_pair(
                    lambda: _time_calls(lambda: ops.linear(x32, w3, None, **qkv), iters),
                    lambda: _time_calls(lambda: ops.linear(x32, w3, None, batch_invariant=True, **qkv), iters), reps=3)
                gemms[f"{tag} out M={rows_ * L} N={C} K={C} bias"] = _median_pair(
                    lambda: _time_calls(lambda: ops.linear(x16, w1, b1), iters),
                    lambda: _time_calls(lambda: ops.linear(x16, w1, b1, batch_invariant=True), iters), reps=3)
                del x32, x16
            r["gemms"] = gemms
            r["gemm_kernels"] = {f"M={m} N={n} K={k}": (ops.linear_kernel_for(m, n, k, bias), ops.linear_kernel_for(m, n, k, bias, True))
                                 for m, n, k, bias in ((B * N * L, 3 * C, C, False), (B * N * L, C, C, True), (B * L, 3 * C, C, False),
                                                       (B * L, C, C, True))}
            rows.append(r)
            torch.cuda.empty_cache()
    return rows


def default_vs_mode_bytes(B=32, L=1024, H=10, N=4):
    """what the mode fixes: identity 0 alone and inside a batch of B, default dispatch and mode (32x32-token class, where the
    default switches kernels between B = 1 and B = 32)"""
    g = torch.Generator().manual_seed(3)
    C = 64 * H
    q = (torch.randn(B, L, C, generator=g) * (0.125 * LOG2E)).to("cuda", torch.bfloat16)
    ks, vs = torch.randn(B, L, C, generator=g).to("cuda", torch.bfloat16), torch.randn(B, L, C, generator=g).to("cuda", torch.bfloat16)
    rk, rv = torch.randn(B, N, L, C, generator=g).to("cuda", torch.bfloat16), torch.randn(B, N, L, C, generator=g).to("cuda", torch.bfloat16)
    aff = ops.adain_stats(vs, rv, heads=H)
    a1 = ops.adain_stats(vs[:1], rv[:1], heads=H)
    for bi in (False, True):
        kw = dict(heads=H, scale=0.125, include_self=True, q_prescaled=True, batch_invariant=bi)
        full = ops.shared_attention(q, ks, vs, rk, rv, adain=aff, **kw)
        one = ops.shared_attention(q[:1], ks[:1], vs[:1], rk[:1], rv[:1], adain=a1, **kw)
        d = (full[:1].float() - one.float()).abs().max().item()
        print(f"identity 0 alone vs in B = {B} (L {L}, H {H}), {'batch-invariant' if bi else 'default        '}: "
              f"{'same bytes' if torch.equal(full[:1], one) else 'DIFFERENT bytes'} (max |diff| {d:.3e})")


def run(cfg):
    dev = torch.device("cuda", 0)
    layers, (B, N, px, dtype, use_adain) = bench.build_workload(cfg, True, dev, seed=1234)
    bench._AUTOCAST["dtype"] = dtype
    for on in (False, True, False, True):   # warm-up of both modes (folded weights, first launches)
        set_mode(layers, on)
        time_steps(layers, B, N, 2)
    ta, tb = [], []
    for r in range(ROUNDS):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            set_mode(layers, on)
            (tb if on else ta).append(time_steps(layers, B, N, STEPS))
    set_mode(layers, False)
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(f"== {cfg}: B = {B}, N = {N}, {px} px, {str(dtype).replace('torch.', '')}, {ROUNDS} alternating rounds x {STEPS} eager steps")
    print(f"step ms   default {ma:.3f} (min {min(ta):.3f} max {max(ta):.3f})   batch-invariant {mb:.3f} (min {min(tb):.3f} max {max(tb):.3f})"
          f"   ratio {mb / ma:.3f}")
    print("per layer class, ms per call (median of alternating repeats of 20 calls), default -> batch-invariant; x3 = the class's three layers:")
    tot = [0.0, 0.0, 0.0]   # added ms per step: shared attention, capture attention, GEMMs
    for r in class_times(layers, B, N, dtype):
        L, H = r["L"], r["H"]
        (sa, sb), (ca, cb) = r["shared"], r["capture"]
        tot[0] += 3 * (sb - sa)
        tot[1] += 3 * (cb - ca)
        print(f"  L {L:5d} H {H:2d}")
        print(f"    shared attention   {sa:.4f} -> {sb:.4f} (x{sb / sa:.3f}); mode: {r['shared_ws']['pieces_per_item']} pieces per "
              f"{r['shared_ws']['rows_per_item']}-row item, per-call scratch {r['shared_ws']['workspace_bytes'] / 1e6:.1f} MB")
        print(f"      default: {r['shared_names'][0]}")
        print(f"      mode   : {r['shared_names'][1]}")
        print(f"    capture attention  {ca:.4f} -> {cb:.4f} (x{cb / ca:.3f}); B*N = {B * N} sets, mode: "
              f"{r['capture_ws']['pieces_per_item']} piece(s) per item, per-call scratch {r['capture_ws']['workspace_bytes'] / 1e6:.1f} MB")
        for name, (ga, gb) in r["gemms"].items():
            tot[2] += 3 * (gb - ga)
            print(f"    GEMM {name:38s} {ga:.4f} -> {gb:.4f} (x{gb / ga:.3f})")
        print("    GEMM kernels (IR_LIN_*: default, mode): " + ", ".join(f"{k}: {v[0]}, {v[1]}" for k, v in r["gemm_kernels"].items()))
    print(f"added per step (x3 layers per class): shared attention {tot[0]:+.3f} ms, capture attention {tot[1]:+.3f} ms, GEMMs {tot[2]:+.3f} ms;"
          f" sum {sum(tot):+.3f} of the step's {mb - ma:+.3f} ms")
    sys.stdout.flush()
    del layers
    torch.cuda.empty_cache()


if __name__ == "__main__":
    default_vs_mode_bytes()
    for cfg in sys.argv[1:] or ["cfg2", "cfg1gpu"]:
        run(cfg)
