#!/usr/bin/env python3
"""bench.py - throughput of the InstantRestore hot path on MI355X.

One "step" = one pass of the hot path over one batch of
synthetic inputs already resident in HBM:

  1. K/V capture (a-3): the nine decoder self-attention layers of the frozen reference UNet over
     the B*N reference token sets - ``AttnProcessor`` = to_q/k/v + fused plain attention + to_out,
     stashing K/V;
  2. harvest (a-4): re-view the stashes as (B,N,L,C) and zero-fill invalid references;
  3. shared attention (a-1, a-2): the nine decoder layers of the main UNet over the B degraded
     images - ``SharedAttnProcessor`` = to_q/k/v + AdaIN statistics + fused extended attention
     (AdaIN folded) + to_out.

Conv/ResNet/VAE stages of the UNets are stock MIOpen/hipBLASLt work outside the path
(OUT OF SCOPE) and are NOT in the step; ``config.workload`` says so.
``value`` = identities (restored images) per second over all ranks = B_total / step time.

Inputs are what the reference's caller hands the processors (inference/test.py:61-83): fp32 module weights, fp32
token activations (LayerNorm output), ``torch.autocast`` to the 16-bit compute dtype - the cast to 16 bit is part of the
step.  The timed steps REPLAY one hipGraph of the two-stream step (captured once during warm-up: same launches, same work,
no CPU launch gaps; ``--graph 0`` times eager launches, and a failed capture falls back to them and says so).

A plain run sets up, warms up, times the K steps, writes the last step's outputs if ``--dump-outputs DIR`` is given and
prints the line (``roofline``, ``cpu_baseline`` and ``config.extras`` null).  With ``--full`` the line also carries the
roofline block, the CPU baseline and, labelled, under ``config.extras``: the same step with eager launches on one and on two
streams, a second graph capture compared bit for bit with eager, the step with cached reference K/V, an
end-to-end leg on the attention-topology host with the stage names of pix2pix_turbo.py:288-336, and the batch
scatter / gather of SURVEY 8e over the process group (RCCL when N > 1).  None of them is ``value``.

Contract: ``python bench.py --gpus N --steps K --warmup W``; for N > 1 launched by
``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...``; one rank per GPU,
identities sharded across ranks (no data-path collective: they are independent), barrier +
synchronize around EXACTLY K timed steps, MAX over ranks, one JSON line from rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch
import torch.distributed as dist

CONFIGS = {
    # name: (identities per GPU, refs, px, dtype, use_adain)
    "cfg2": (8, 4, 512, "bf16", True),    # BASELINE.json configs[1]: the configuration the metric is quoted on
    "cfg4": (8, 8, 512, "bf16", True),    # 8 references
    "cfg5": (16, 4, 1024, "f16", True),   # 1024 px
    "cfg1gpu": (1, 4, 512, "f16", True),  # configs[0]'s shape on the GPU: ONE identity under fp16 autocast, the way inference/test.py:79-111
                                          # drives the model - launch-bound: what the host side costs per layer shows here
}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_workload(cfg, train_input, dev, seed, act_fp32=True):
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    from instantrestore_amd.roofline import layer_classes

    B, N, px, dt, use_adain = CONFIGS[cfg]
    dtype = DT[dt]
    g = torch.Generator(device="cpu").manual_seed(seed)
    layers = []
    idx = 0
    # the modules' default initialisation (the to_out bias keeps it) draws from torch's global CPU generator: seeded here as
    # well, so that the same arguments give the same inputs run to run; the caller's CPU generator state is left as it was
    # and no device generator is touched
    with torch.random.fork_rng(devices=[]):
        torch.default_generator.manual_seed(seed)     # the CPU generator only: the modules are initialised on the CPU
        for (L, C, H) in layer_classes(px):
            for _ in range(3):
                def mk(proc):
                    a = Attention(query_dim=C, heads=H, dim_head=64, processor=proc)
                    with torch.no_grad():
                        for lin in (a.to_q, a.to_k, a.to_v, a.to_out[0]):
                            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / C ** 0.5)
                    return a.to(dev) if act_fp32 else a.to(dev, dtype)   # test.py:61-63: the model stays fp32 under autocast
                kv_attn = mk(AttnProcessor())
                main_attn = mk(SharedAttnProcessor(self_attn_idx=idx, use_adain=use_adain, train_input=train_input))
                # token activations entering the two attentions (LayerNorm output in the real UNet)
                act = torch.float32 if act_fp32 else dtype
                h_ref = torch.randn(B * N, L, C, generator=g).to(dev, act)
                h_main = torch.randn(B, L, C, generator=g).to(dev, act)
                layers.append(dict(L=L, C=C, H=H, kv_attn=kv_attn, main_attn=main_attn, h_ref=h_ref, h_main=h_main))
                idx += 1
    return layers, (B, N, px, dtype, use_adain)


_REF_STREAM = {}


REF_STATS = {"on": True}      # A/B switch: False = every shared layer re-reads all reference V's for its AdaIN statistics also on one stream
_AUTOCAST = {"dtype": None}   # set by main(): the 16-bit compute dtype the step autocasts to (None: inputs already 16 bit)


def hot_path_step(layers, B, N, ref_early_exit=False, two_streams=False, cached_kv=None, return_kv=False):
    if _AUTOCAST["dtype"] is None:
        return _hot_path_step(layers, B, N, ref_early_exit, two_streams, cached_kv, return_kv)
    with torch.autocast("cuda", dtype=_AUTOCAST["dtype"]):
        return _hot_path_step(layers, B, N, ref_early_exit, two_streams, cached_kv, return_kv)


def _hot_path_step(layers, B, N, ref_early_exit=False, two_streams=False, cached_kv=None, return_kv=False):
    """one pass: K/V capture -> harvest -> shared attention.  Returns the 9 outputs.
    ``cached_kv`` = (keys, values): the reference branch is skipped (per-identity K/V cache).

    ``two_streams``: the reference UNet's layers run on their own HIP stream and shared layer i waits only
    for the event of capture layer i (it reads nothing else), so the small layer classes - which cannot
    fill 256 CUs on their own - overlap with the other UNet's kernels.  Same kernels, same work."""
    from instantrestore_amd.attn_processors import ReferenceCaptureComplete
    if cached_kv is not None:
        keys, vals, stats = (cached_kv[0], cached_kv[1], cached_kv[2] if len(cached_kv) > 2 else None)
        rvalid = cached_kv[3] if len(cached_kv) > 3 else None    # int32 (B,): references n >= valid[b] are zero-filled (ABI v8)
        return [ly["main_attn"](ly["h_main"], ref_keys=keys, ref_values=vals, ref_stats=stats, ref_valid=rvalid) for ly in layers]
    cur = torch.cuda.current_stream()
    ref_stream = cur
    if two_streams:
        ref_stream = _REF_STREAM.setdefault(cur.device, torch.cuda.Stream(device=cur.device))
        ref_stream.wait_stream(cur)
    # 1. K/V capture on the reference token sets (--ref-early-exit: the reference UNet stops after to_k / to_v
    #    of its last capturing layer, SURVEY 8f rank 2 - NOT the default, the headline runs all nine in full)
    procs = [ly["kv_attn"].processor for ly in layers]
    for p in procs:
        p.stop_after_capture = procs if ref_early_exit else None
    # AdaIN content statistics (mean / std of every reference V) once per reference, in the capture layer.  Round 4: they are
    # the tail of that layer's q/k/v GEMM (ir_linear_fwd_stats: no pass over V), so they ride on the capture stream for free;
    # with the tail off (attn_processors.FUSED_STATS = False, the round-3 A/B) the standalone pass would lengthen the capture
    # stream - the longer one of the two - by 0.3 ms (profiles/r3_ab_step.txt) and the shared layers keep it instead
    from instantrestore_amd import attn_processors as _ap_mod
    use_stats = bool(layers[0]["main_attn"].processor.use_adain) and REF_STATS["on"] and (_ap_mod.FUSED_STATS or not two_streams)
    for p in procs:
        p.record_events = two_streams
        p.capture_stats = use_stats    # AdaIN content statistics once per reference, on the capture stream (kv_harvest)
    with torch.cuda.stream(ref_stream):
        for ly in layers:
            try:
                ly["kv_attn"](ly["h_ref"])
            except ReferenceCaptureComplete:
                pass
    # 2. harvest (views) + zero-fill of invalid references (valid = N at inference, test.py:81)
    keys, vals, events, stats = [], [], [], []
    for ly in layers:
        p = ly["kv_attn"].processor
        keys.append(p.keys.reshape(-1, N, p.keys.shape[1], p.keys.shape[2]))
        vals.append(p.values.reshape(-1, N, p.values.shape[1], p.values.shape[2]))
        if p.v_part is not None:    # round 4: content statistics as the capture GEMM's partials, merged by the shared layer's affine kernel
            from instantrestore_amd import ops as _o
            stats.append(_o.RefStatsPartials(p.v_part, p.values.shape[0] // N, N, p.values.shape[1], producer=p.stream))
        else:
            stats.append(None if p.v_mean is None else (p.v_mean.reshape(-1, N, *p.v_mean.shape[-2:]), p.v_std.reshape(-1, N, *p.v_std.shape[-2:])))
        events.append(p.ready)
        p.reset()
    # 3. shared attention on the degraded images (each layer waits for its own reference layer's event)
    outs = []
    for ly in layers:
        outs.append(ly["main_attn"](ly["h_main"], ref_keys=keys, ref_values=vals,
                                    ref_events=events if two_streams else None, ref_stats=stats if use_stats else None))
    if two_streams:
        cur.wait_stream(ref_stream)
    if return_kv:      # determinism checks compare the harvested K/V lists too
        return outs, keys, vals
    return outs


def measure_roofline(layers, B, N, train_input, use_adain, dtype):
    """dominant kernel = fused shared attention of the 64x64-token layer class; timed live with
    HIP events on the launch stream (ir_time_shared_attn_fwd)."""
    from instantrestore_amd import ops
    from instantrestore_amd.roofline import MFMA_PEAK_TFLOPS_16BIT, attn_bytes, attn_flops

    ly = layers[-1]
    L, C, H = ly["L"], ly["C"], ly["H"]
    a = ly["main_attn"]
    with torch.no_grad():
        from instantrestore_amd import attn_processors as ap
        hm, hr = ly["h_main"].to(dtype), ly["h_ref"].to(dtype)
        lin = lambda m, x: torch.nn.functional.linear(x, m.weight.to(dtype))
        k, v = lin(a.to_k, hm), lin(a.to_v, hm)
        # q exactly as the processor produces it at this shape: through the library's own fused-projection GEMM it
        # leaves the epilogue pre-scaled (attn_processors._project_qkv) and the attention runs its pre-scaled-Q form
        wq = a.to_q.weight.to(dtype)
        presc = bool(ap.PRESCALE_Q and ap._own_gemm(hm, torch.cat([wq, wq, wq], 0), None))
        q = ops.linear(hm, wq, None, scale_cols=C, col_scale=0.125 * ap.LOG2E) if presc else lin(a.to_q, hm)
        kr = lin(layers[-1]["kv_attn"].to_k, hr).reshape(B, N, L, C)
        vr = lin(layers[-1]["kv_attn"].to_v, hr).reshape(B, N, L, C)
        aff = ops.adain_stats(v, vr, heads=H) if use_adain else None
        kw = dict(heads=H, scale=0.125, include_self=train_input, adain=aff, q_prescaled=presc)
        ops.time_shared_attention(q, k, v, kr, vr, iters=3, **kw)
        ms = ops.time_shared_attention(q, k, v, kr, vr, iters=20, **kw)
        kname = ops.shared_attention_kernel_name(q, k, v, kr, vr, **kw)
    lkv = (N + int(train_input)) * L
    flops = attn_flops(B, L, lkv, C)
    tf = flops / (ms * 1e-3) / 1e12
    return {
        "bound": "mfma",
        "kernel": "%s %s (L=%d, Lkv=%d, H=%d, B=%d)" % (
            kname, {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype], L, lkv, H, B),
        "achieved": round(tf, 2),
        "peak": MFMA_PEAK_TFLOPS_16BIT,
        "unit": "TFLOP/s",
        "frac": round(tf / MFMA_PEAK_TFLOPS_16BIT, 4),
        "ms_per_launch": round(ms, 4),
        "algorithmic_gflop_per_launch": round(flops / 1e9, 2),
        "algorithmic_mb_per_launch": round(attn_bytes(B, L, lkv, C) / 1e6, 2),
        # HBM bytes per launch from a separate rocprofv3 --pmc pass of this kernel at this shape
        # (tools/pmc_attn.sh -> profiles/r3_pmc_shared_attn.txt, the r2_ / r1_ files if absent); FETCH_SIZE doubled per the
        # gfx950 correction of MI355X_MICROARCH.md.  null if the profile is not for this shape.
        "traffic": _pmc_traffic_bytes() if (B, N, L, H, train_input, use_adain) == (8, 4, 4096, 5, True, True) else None,
        "traffic_static": True,      # read from the committed PMC pass named below, NOT measured in this run (counters need rocprofv3)
        "traffic_unit": "bytes/launch (PMC: 2*FETCH_SIZE + WRITE_SIZE, %s)" % _pmc_profile_name(),
        "power_note": "this kernel runs at the 1400 W board cap on random data: round 6's 128-row kernel needs 1.39 M cycles per launch "
                      "(the 64-row kernel 1.77 M) and is clocked at 1.96 GHz (2.24 GHz) against the 2.4 GHz the peak assumes - 0.99 J per "
                      "launch (1.10 J) - profiles/r6_pmc_w128.txt, r6_w128_ab.txt; an MFMA-only stream of the same instruction holds "
                      "1.92-1.97 PFLOP/s on random operands under that cap (at_power_cap below, measured in this run)",
    }


def kernel_class_breakdown(layers, B, N, steps):
    """GPU time of one step by kernel class, from HIP events recorded on the launch stream around every call into the
    library during ``steps`` one-stream steps (the wrappers of ``instantrestore_amd.ops`` the processors call are
    patched for the duration).  ms per step and share of the summed GPU time; classes: fused attention per token-axis
    class (shared = over [self] ++ references, capture = plain self-attention of the reference token sets),
    projection GEMMs per K, AdaIN statistics."""
    from instantrestore_amd import ops
    rec = []

    def timed(fn, label):
        def w(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            rec.append((label(*a, **kw), e0, e1))
            return r
        return w

    # algorithmic work of every call beside its label: attention 4*B*Lq*Lkv*C flops, GEMM 2*M*N*K flops,
    # AdaIN statistics the bytes of the V matrices the call reads once
    work = {}

    def note(label, flops=0.0, nbytes=0.0):
        f, b = work.get(label, (0.0, 0.0))
        work[label] = (f + flops, b + nbytes)
        return label

    def att_label(q, k, v, rk=None, rv=None, **kw):
        lkv = (k.shape[1] if kw.get("include_self", True) or rk is None else 0) + (0 if rk is None else rk.shape[1] * rk.shape[2])
        return note("attention L=%d %s" % (q.shape[1], "shared" if rk is not None else "capture"),
                    flops=4.0 * q.shape[0] * q.shape[1] * lkv * q.shape[2])

    def lin_label(x, w, b=None, **kw):
        rows = x.numel() // x.shape[-1]
        return note("projection GEMM K=%d" % w.shape[1], flops=2.0 * rows * w.shape[0] * w.shape[1],
                    nbytes=float(x.numel() * x.element_size() + w.numel() * w.element_size() + rows * w.shape[0] * w.element_size()))

    saved = (ops.shared_attention, ops.linear, ops.adain_stats, ops.adain_stats_cached, ops.token_stats,
             ops.adain_affine_from_partials, ops.token_stats_from_partials)
    ops.shared_attention = timed(saved[0], att_label)
    ops.linear = timed(saved[1], lin_label)
    ops.adain_stats = timed(saved[2], lambda v, rv, **kw: note("AdaIN statistics", nbytes=2.0 * (v.numel() + rv.numel())))
    ops.adain_stats_cached = timed(saved[3], lambda v, m, sd, **kw: note("AdaIN statistics", nbytes=2.0 * v.numel()))
    ops.token_stats = timed(saved[4], lambda x, **kw: note("AdaIN statistics", nbytes=2.0 * x.numel()))
    # round 4: the statistics are the q/k/v GEMMs' tail (inside "projection GEMM"); what is left are the merges of the partials
    ops.adain_affine_from_partials = timed(saved[5], lambda st, *a, **kw: note("AdaIN affine from GEMM partials", nbytes=4.0 * st.ws.numel()))
    ops.token_stats_from_partials = timed(saved[6], lambda st, *a, **kw: note("AdaIN affine from GEMM partials", nbytes=4.0 * st.ws.numel()))
    try:
        with torch.no_grad():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                hot_path_step(layers, B, N, False, False)
            torch.cuda.synchronize()
            t_instr = (time.perf_counter() - t0) / steps * 1e3
    finally:
        (ops.shared_attention, ops.linear, ops.adain_stats, ops.adain_stats_cached, ops.token_stats,
         ops.adain_affine_from_partials, ops.token_stats_from_partials) = saved
    # the same one-stream step WITHOUT the event pairs: what the classes must add up to.  An event record between two
    # kernels costs the stream a few us (round 3: the classes summed to 7.40 ms of a 7.21 ms step); the per-class times
    # below are scaled by plain / instrumented so that they are shares of the step as it runs un-instrumented
    with torch.no_grad():
        t_plain = _time_steps(lambda: hot_path_step(layers, B, N, False, False), steps, warm=1) * 1e3
    tot = {}
    for label, e0, e1 in rec:
        tot[label] = tot.get(label, 0.0) + e0.elapsed_time(e1)
    allms = sum(tot.values())
    scale = min(1.0, t_plain / t_instr) if t_instr > 0 else 1.0
    out = {}
    for k, v in sorted(tot.items(), key=lambda kv: -kv[1]):
        v = v * scale
        row = {"ms_per_step": round(v / steps, 4), "share": round(v / (allms * scale), 4)}
        f, b = work.get(k, (0.0, 0.0))
        if f:
            row["tflops"] = round(f / v / 1e9, 1)
            row["frac_of_mfma_peak"] = round(f / v / 1e9 / 2500.0, 4)
        if b:
            row["gb_per_s"] = round(b / v / 1e6, 1)
            row["frac_of_hbm_peak"] = round(b / v / 1e6 / 8000.0, 4)
        if f and b:
            # which roofline binds the class: its algorithmic flops at the 2.5 PF MFMA peak against its algorithmic bytes at
            # the 8 TB/s HBM peak (ridge = 312 FLOP/B).  K = 320 projections: 190-210 FLOP/B, below the ridge -> HBM
            t_mfma, t_hbm = f / 2500e12, b / 8e12
            row["bound"] = "hbm" if t_hbm > t_mfma else "mfma"
            row["flop_per_byte"] = round(f / b, 1)
            row["frac_of_roofline"] = round(max(t_mfma, t_hbm) * 1e3 / v, 4)
        out[k] = row
    # context for the HBM-bound classes: what a plain device-to-device copy sustains on this box right now (1 GiB read +
    # 1 GiB written per pass; the guide's 8 TB/s is the pin rate) - informational, next to the contract's frac_of_hbm_peak
    try:
        src = torch.empty(1 << 28, dtype=torch.float32, device=layers[0]["h_main"].device)
        dst = torch.empty_like(src)
        for _ in range(2):
            dst.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copy_gbs = 8 * 2 * src.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        del src, dst
        for row in out.values():
            if row.get("bound") == "hbm":
                row["frac_of_measured_copy"] = round(row["gb_per_s"] / copy_gbs, 4)
        out["_hbm_copy_gb_per_s_measured"] = round(copy_gbs, 1)
    except Exception:
        pass
    out["_reconciliation"] = {"classes_sum_ms": round(allms * scale / steps, 4), "one_stream_step_ms_plain": round(t_plain, 4),
                              "one_stream_step_ms_with_events": round(t_instr, 4), "scale_applied": round(scale, 4),
                              "note": "class times = HIP-event times x (plain step / instrumented step): the event pairs cost the "
                                      "stream time that is not the kernels'; what the scaled classes leave of the plain step is launch gaps"}
    return out


def _pmc_profile_name():
    for name in ("r6_pmc_shared_attn.txt", "r5_pmc_shared_attn.txt", "r4_pmc_shared_attn.txt", "r3_pmc_shared_attn.txt", "r2_pmc_shared_attn.txt", "r1_pmc_shared_attn.txt"):
        if os.path.exists(os.path.join(REPO, "profiles", name)):
            return "profiles/" + name
    return "no committed PMC profile"


def _pmc_traffic_bytes():
    import ast
    path = os.path.join(REPO, _pmc_profile_name())
    try:
        vals = {}
        for line in open(path):
            i, j = line.find("{"), line.rfind("}")
            if i >= 0 and j > i:
                vals.update(ast.literal_eval(line[i:j + 1]))
        return int((2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024)
    except Exception:
        return None


def live_pmc_traffic(timeout_s=150):
    """OPT-IN (``IR_BENCH_LIVE_PMC=1``): HBM bytes per launch of the dominant kernel measured in THIS run - two counter-only
    ``rocprofv3 --pmc`` passes (FETCH_SIZE, then WRITE_SIZE; never together with a trace domain beyond --kernel-trace) of
    ``tools/prof_attn.py`` at the cfg-2 top-layer shape as child processes, each under its own timeout, with the guide's gfx950
    correction (2 * FETCH_SIZE + WRITE_SIZE, KiB).  Off by default: counter collection is the one thing on this pool that has hung
    a box before (the TCC_EA0 pass, NOTES 11.1), and the driver's bench run must never depend on it; the committed pass
    (``traffic_static``) stays the default source.  Returns (bytes, detail) or (None, reason)."""
    import csv, glob, shutil, subprocess, tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        out = tempfile.mkdtemp(prefix="ir_pmc_", dir="/tmp")
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "-o", counter.lower(), "--",
               sys.executable, os.path.join(REPO, "tools", "prof_attn.py"), "0", "3", "4096", "5", "1", "1", "1"]
        import signal
        proc = subprocess.Popen(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                start_new_session=True)
        try:
            log, _ = proc.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            try:
                os.killpg(proc.pid, signal.SIGKILL)      # the profiler AND the workload it spawned (its own session: exactly this group)
            except OSError:
                pass
            proc.wait()
            return None, "%s pass timed out after %d s" % (counter, timeout_s)
        if proc.returncode != 0:
            return None, "%s pass failed: %s" % (counter, (log or "")[-200:])
        got = []
        for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "shared_attn_fwd_w64" in row["Kernel_Name"] and row["Counter_Name"] == counter:
                    got.append(float(row["Counter_Value"]))
        shutil.rmtree(out, ignore_errors=True)
        if not got:
            return None, "%s: no row of the kernel in the counter file" % counter
        vals[counter] = sum(got) / len(got)
    return int((2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024), {"FETCH_SIZE_KiB": round(vals["FETCH_SIZE"], 1),
                                                                          "WRITE_SIZE_KiB": round(vals["WRITE_SIZE"], 1), "launches": 3}


def baseline_layer(L, C, N, dtype=None):
    """one layer of the CPU baseline / deviation report: four projection weights and the activations of the N reference token
    sets and of the degraded image, rounded to values the device path's 16-bit type holds exactly (so both sides start equal)"""
    r16 = (lambda t: t.to(dtype).float()) if dtype is not None else (lambda t: t)
    w = [r16(torch.randn(C, C) / C ** 0.5) for _ in range(4)]
    return dict(w=w, bo=torch.zeros(C), h_ref=r16(torch.randn(N, L, C)), h_main=r16(torch.randn(1, L, C)))


def baseline_pass(ly, H, N, adain, t_in):
    """the oracle's fp32 torch-CPU port of the reference operator sequence on one layer: K/V capture over the N reference token
    sets, then the shared layer.  Returns (seconds, output)."""
    from oracle import shared_attn_oracle as O
    w, bo = ly["w"], ly["bo"]
    L, C = ly["h_main"].shape[1:]
    t0 = time.perf_counter()
    O.shared_attn_processor_port(ly["h_ref"], w[0], w[1], w[2], w[3], bo, None, None, H)       # K/V capture over the N reference token sets
    kr = torch.nn.functional.linear(ly["h_ref"], w[1]).reshape(1, N, L, C)
    vr = torch.nn.functional.linear(ly["h_ref"], w[2]).reshape(1, N, L, C)
    out = O.shared_attn_processor_port(ly["h_main"], w[0], w[1], w[2], w[3], bo, kr, vr, H, adain, t_in)
    return time.perf_counter() - t0, out


def device_path_deviation(ly, H, N, use_adain, train_input, dtype, dev):
    """the same layer pair through the product path (K/V-capturing processor -> harvest -> shared processor under autocast)
    on the GPU, against the port's fp32 result ``ly["port_out"]``: SURVEY 8d's "max-abs deviation vs the CPU restatement per
    dtype".  Returns (max|device - port|, max|port|).  tests/test_gpu_deviation.py holds it to 2.5e-3 (bf16) / 3e-4 (fp16)."""
    from types import SimpleNamespace
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    from instantrestore_amd.kv_harvest import harvest_reference_kv
    C = ly["h_main"].shape[2]

    def mk(proc):
        a = Attention(query_dim=C, heads=H, dim_head=64, processor=proc)
        with torch.no_grad():
            for lin, w in zip((a.to_q, a.to_k, a.to_v, a.to_out[0]), ly["w"]):
                lin.weight.copy_(w)
            a.to_out[0].bias.zero_()
        return a.to(dev)
    cap, main = mk(AttnProcessor()), mk(SharedAttnProcessor(self_attn_idx=0, use_adain=use_adain, train_input=train_input))
    fake = SimpleNamespace(attn_processors={"up_blocks.1.attentions.0.transformer_blocks.0.attn1.processor": cap.processor})
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        cap(ly["h_ref"].to(dev))
        keys, values = harvest_reference_kv(fake, N, [N])[:2]
        out = main(ly["h_main"].to(dev), ref_keys=keys, ref_values=values)
    ref = ly["port_out"]
    return float((out.float().cpu() - ref).abs().max()), float(ref.abs().max())


def cpu_baseline(N, px, train_input, use_adain, seed, budget_s=28.0, reps=3, dtype=None, dev=None):
    """oracle port (torch-CPU fp32, the reference's operator sequence) on the host cores: one identity through the same
    9 + 9 layers.  SURVEY 8d: ALL nine layer shapes (three per class, each with its own weights and activations, not one
    counted three times), 1 warm-up per class + the median of ``reps`` timed passes per layer for the configuration's own
    (use_adain, train_input), and one timed pass per layer of the OTHER flag setting (AdaIN off, no self block) beside it;
    bounded to ~budget_s of CPU work (fewer repetitions on a slow host, stated in `sample`)."""
    from instantrestore_amd.roofline import layer_classes
    from oracle import shared_attn_oracle as O

    torch.manual_seed(seed)
    cores = torch.get_num_threads()

    make_layer = lambda L, C: baseline_layer(L, C, N, dtype)

    def one_pass(ly, H, adain, t_in):
        dt, out = baseline_pass(ly, H, N, adain, t_in)
        if adain == use_adain and t_in == train_input:
            ly["port_out"] = out          # kept for the deviation report below (the oracle as the CHECKER of the device path)
        return dt

    device_deviation = lambda ly, H: device_path_deviation(ly, H, N, use_adain, train_input, dtype, dev)

    spent = 0.0
    per_layer, other, reps_done = [], [], []
    all_layers = []
    classes = layer_classes(px)
    for ci, (L, C, H) in enumerate(classes):
        layers3 = [make_layer(L, C) for _ in range(3)]
        all_layers.extend(layers3)
        spent += one_pass(layers3[0], H, use_adain, train_input)            # warm-up of the class (allocator, thread pool)
        for ly in layers3:
            times = []
            for _ in range(reps):
                # a repetition beyond the first only while the class stays inside its share of the budget (the classes cost
                # ~1 : 2.3 : 7 per layer; what follows - the remaining layers, the other setting - needs the rest)
                if times and spent + times[0] > budget_s * (0.45 + 0.15 * ci):
                    break
                dt = one_pass(ly, H, use_adain, train_input)
                spent += dt
                times.append(dt)
            per_layer.append(sorted(times)[len(times) // 2])
            reps_done.append(len(times))
        for ly in layers3:
            if spent > budget_s * 1.2:
                other.append(None)
                continue
            dt = one_pass(ly, H, False, False)
            spent += dt
            other.append(dt)
    t_total = sum(per_layer)
    t_other = sum(t for t in other if t is not None) if all(t is not None for t in other) else None
    deviation = None
    if dtype is not None and dev is not None:
        try:
            per_class, li = [], 0
            for (L, C, H) in classes:
                errs = [device_deviation(ly, H) for ly in all_layers[li:li + 3]]
                li += 3
                per_class.append({"L": L, "H": H, "max_abs_err": float("%.3e" % max(e for e, _ in errs)), "max_abs_ref": round(max(r for _, r in errs), 3)})
            worst = max(c["max_abs_err"] / max(1.0, c["max_abs_ref"]) for c in per_class)
            deviation = {"dtype": str(dtype).replace("torch.", ""), "layer_classes": per_class,
                         "max_abs_err": max(c["max_abs_err"] for c in per_class), "worst_err_over_max_1_ref": float("%.3e" % worst),
                         "note": "device path (capture processor -> harvest -> shared processor, autocast) against the fp32 port of the reference "
                                 "operator sequence on the SAME 16-bit-representable weights and activations, one identity, all nine layers; "
                                 "includes the 16-bit rounding of q / k / v, of the K/V stash and of the attention output on the device "
                                 "(tests/test_gpu_deviation.py holds this level to 2.5e-3 (bf16) / 3e-4 (fp16))"}
        except Exception as e:   # a report, never a reason to lose the line
            deviation = {"error": repr(e)[:300]}
    return {
        "value": round(1.0 / t_total, 4) if t_total > 0 else None,
        "unit": "images/s",
        "cores": cores,
        "kind": "port",
        "deviation_of_device_path": deviation,
        "other_setting": {"use_adain": False, "train_input": False,
                          "value": None if not t_other else round(1.0 / t_other, 4),
                          "seconds_per_layer": [None if t is None else round(t, 3) for t in other]},
        "sample": "1 identity, %d refs, %d px, fp32 torch-CPU port of the reference operator sequence "
                  "(oracle/shared_attn_oracle.py), %s; all nine layers timed (capture over the N reference token sets + shared "
                  "layer; 1 warm-up per class, median of %s passes per layer; use_adain=%s, train_input=%s), then one pass per "
                  "layer with AdaIN off and no self block (`other_setting`); seconds per layer: %s; %.0f s of CPU work"
                  % (N, px, torch.__config__.parallel_info().split("\n")[1].strip(), reps_done, use_adain, train_input,
                     [round(t, 3) for t in per_layer], spent),
    }


# ---------------------------------------------------------------------------------------------------------------------
# labelled extras next to the headline (never `value`)
# ---------------------------------------------------------------------------------------------------------------------
def _time_steps(fn, steps, warm=3):
    for _ in range(warm):   # the GPU sat idle during the CPU baseline: bring clocks and caches back before timing
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def power_probe(step_fn, seconds=3.0):
    """board power and shader clock while the step runs back to back for `seconds` (rocm-smi from a side thread): the step
    is power-capped on random data, and the clock the kernels get is what the cap leaves - the roofline peaks are quoted at
    the 2.4 GHz the chip only holds on idle-ish or all-zero workloads"""
    import shutil
    import subprocess
    import threading
    smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(smi):
        return {"error": "rocm-smi not found"}
    samples, stop = [], []

    def sampler():
        while not stop:
            try:
                out = subprocess.run([smi, "--showpower", "--showclocks", "--csv"], capture_output=True, text=True, timeout=10).stdout
                rows = [r for r in out.strip().splitlines() if r.strip()]
                head, vals = rows[0].split(","), rows[1].split(",")
                rec = dict(zip(head, vals))
                w = [float(v) for k, v in rec.items() if "Power" in k and v.replace(".", "", 1).isdigit()]
                c = [float(v.strip("()").lower().replace("mhz", "")) for k, v in rec.items() if k.startswith("sclk clock speed")]
                if w and c:
                    samples.append((w[0], c[0]))
            except Exception:   # a sample lost is a sample lost
                pass
            time.sleep(0.2)

    for _ in range(3):
        step_fn()
    torch.cuda.synchronize()
    th = threading.Thread(target=sampler, daemon=True)
    th.start()
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            step_fn()
        n += 10
        torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / n
    stop.append(1)
    th.join(timeout=15)
    body = samples[1:] if len(samples) > 2 else samples    # the first sample may predate the load
    if not body:
        return {"error": "no rocm-smi sample parsed", "ms_per_step_sustained": round(sec * 1e3, 4)}
    return {"watts_avg": round(sum(w for w, _ in body) / len(body), 1), "watts_max": round(max(w for w, _ in body), 1),
            "sclk_mhz_avg": round(sum(c for _, c in body) / len(body), 1), "samples": len(body),
            "ms_per_step_sustained": round(sec * 1e3, 4), "steps": n, "board_cap_watts": 1400, "sclk_peak_mhz": 2400,
            "note": "%.0f s of back-to-back steps with rocm-smi sampled beside them; roofline peaks assume 2.4 GHz" % seconds}


class CapturedStep:
    """the whole two-stream step captured once in ONE hipGraph (fork / join through the processors' events) with the product's
    own helper, ``kv_harvest.capture_step``; ``replay()`` re-runs it, ``outs`` / ``keys`` / ``vals`` are the graph's static
    result tensors"""

    def __init__(self, layers, B, N, two_streams=True):
        from instantrestore_amd.kv_harvest import capture_step
        saved = dict(_REF_STREAM)
        _REF_STREAM.clear()       # the side stream (and the per-stream workspaces) are created by the helper's eager warm-up run
        try:
            self._cap = capture_step(lambda: hot_path_step(layers, B, N, False, two_streams, return_kv=True), warmup=1)
        finally:
            torch.cuda.synchronize()
            _REF_STREAM.clear()
            _REF_STREAM.update(saved)
        self.graph = self._cap.graph
        self.outs, self.keys, self.vals = self._cap.result

    def replay(self):
        self._cap.replay()


def _first_difference(t, b):
    """where two same-shape tensors first differ (row-major), how many elements do, and the two values there"""
    ne = (t != b).flatten()
    idx = int(ne.nonzero()[0])
    where = []
    rem = idx
    for d in reversed(t.shape):
        where.append(rem % d)
        rem //= d
    return {"elements": int(ne.sum()), "of": int(ne.numel()), "first_index": list(reversed(where)),
            "got": float(t.flatten()[idx].float()), "expected": float(b.flatten()[idx].float()),
            "max_abs": float((t.float() - b.float()).abs().max())}


def determinism_report(layers, B, N, reps=10, modes=("one_stream", "two_streams", "hip_graph")):
    """The step run three ways - one stream, two streams, two streams replayed from one hipGraph - ``reps`` times each;
    every layer output and every harvested K/V tensor is compared bit for bit (``torch.equal``) with the first one-stream
    run.  The reference runs one stream (inference/test.py:79-111), i.e. deterministically: so must every schedule here.
    A mismatch is recorded with everything needed to bisect it: mode, repetition, tensor kind and layer (``out3`` / ``key7`` /
    ``val0``), the layer's (L, C, H), how many elements differ, the first differing index with both values (``details``)."""
    def snap(res):
        outs, keys, vals = res
        return [t.clone() for t in list(outs) + list(keys) + list(vals)]
    n = len(layers)
    names = ["out%d" % i for i in range(n)] + ["key%d" % i for i in range(n)] + ["val%d" % i for i in range(n)]
    base = snap(hot_path_step(layers, B, N, False, False, return_kv=True))
    torch.cuda.synchronize()
    cap = CapturedStep(layers, B, N) if "hip_graph" in modes else None
    runs = {
        "one_stream": lambda: hot_path_step(layers, B, N, False, False, return_kv=True),
        "two_streams": lambda: hot_path_step(layers, B, N, False, True, return_kv=True),
        "hip_graph": lambda: (cap.replay(), (cap.outs, cap.keys, cap.vals))[1],
    }
    report = {}
    for mode in modes:
        fn = runs[mode]
        bad, details = {}, []
        for rep in range(reps):
            got = fn()
            torch.cuda.synchronize()
            for i, (name, t, b) in enumerate(zip(names, list(got[0]) + list(got[1]) + list(got[2]), base)):
                if not torch.equal(t, b):
                    d = _first_difference(t, b)
                    bad[name] = max(bad.get(name, 0.0), d["max_abs"])
                    if len(details) < 8:
                        ly = layers[i % n]
                        details.append(dict(d, mode=mode, repetition=rep, tensor=name, layer=i % n, L=ly["L"], C=ly["C"], H=ly["H"]))
            del got
        report[mode] = {"runs": reps, "identical": not bad, "mismatching": bad, "details": details}
    del cap
    return report


def extra_graph(layers, B, N, steps):
    """the whole two-stream step captured in ONE hipGraph and replayed: same launches, same work, no CPU launch gaps.
    Returns (seconds per replay, bit-identical?, detail): every layer output AND every harvested K/V tensor of three
    replays is compared with a fresh eager two-stream run; a mismatch is reported per tensor together with whether the
    eager run repeats itself (tests/test_gpu_determinism.py asserts all of it)."""
    cap = CapturedStep(layers, B, N)
    for _ in range(2):
        cap.replay()
    sec = _time_steps(cap.replay, steps)
    ref = hot_path_step(layers, B, N, False, True, return_kv=True)
    torch.cuda.synchronize()
    ref = [t.clone() for part in ref for t in part]
    n = len(layers)
    names = ["out%d" % i for i in range(n)] + ["key%d" % i for i in range(n)] + ["val%d" % i for i in range(n)]
    bad = {}
    for _ in range(3):
        cap.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(names, list(cap.outs) + list(cap.keys) + list(cap.vals), ref):
            if not torch.equal(a, b):
                bad[name] = max(bad.get(name, 0.0), float((a.float() - b.float()).abs().max()))
    detail = {"tensors_compared": len(names), "replays_compared": 3}
    if bad:
        again = hot_path_step(layers, B, N, False, True, return_kv=True)
        torch.cuda.synchronize()
        detail.update({"mismatching": bad,
                       "eager_repeats_itself": all(torch.equal(a, b) for a, b in zip([t for part in again for t in part], ref))})
    return sec, not bad, detail


def extra_cfg1gpu(dev, steps, act_fp32):
    """configs[0]'s shape on the GPU - ONE identity, 4 references, 512 px, fp16 autocast: the schedule inference/test.py:79-111
    actually runs (eager, B = 1) - next to the same step replayed from one hipGraph (kv_harvest.capture_step) and the dominant
    kernel's roofline fraction at B = 1 (40 work items of 512 rows on 256 CUs: every item cut into K/V-range pieces)."""
    saved = _AUTOCAST["dtype"]
    layers, (B, N, px, dtype, use_adain) = build_workload("cfg1gpu", True, dev, seed=4321, act_fp32=act_fp32)
    _AUTOCAST["dtype"] = dtype if act_fp32 else None
    try:
        with torch.no_grad():
            for _ in range(3):
                hot_path_step(layers, B, N, False, False)
            sec_e = _time_steps(lambda: hot_path_step(layers, B, N, False, False), steps)
            cap = CapturedStep(layers, B, N, True)
            for _ in range(3):
                cap.replay()
            sec_g = _time_steps(cap.replay, steps)
            roof = measure_roofline(layers, B, N, True, use_adain, dtype)
    finally:
        _AUTOCAST["dtype"] = saved
    return {"workload": "cfg1gpu: 1 identity, %d refs, %d px, %s" % (N, px, {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]),
            "hip_graph": {"images_per_s": round(B / sec_g, 2), "ms_per_step": round(sec_g * 1e3, 4)},
            "eager_one_stream": {"images_per_s": round(B / sec_e, 2), "ms_per_step": round(sec_e * 1e3, 4),
                                 "note": "the reference's own schedule; host-bound (issue time of ~80 launches), NOTES 11.11"},
            "dominant_kernel": {"kernel": roof["kernel"], "ms_per_launch": roof["ms_per_launch"], "achieved": roof["achieved"],
                                "frac": roof["frac"], "unit": "TFLOP/s", "timing": "20 back-to-back launches (HIP events)"}}


def extra_ragged_valid(layers, B, N, keys, vals, cst, sec_all_valid, train_input, steps, dev):
    """Zero-filled references in closed form (ABI v8 ``valid_refs``): the nine shared layers on cached K/V whose references
    ``n >= valid`` were zero-filled like pix2pix_turbo.py:269-273 does (``inference/test.py:81`` passes the CHECKPOINT's
    ``max_conditioning_images``: 4 of the 8 references of the cfg-4 case).  Timed twice per valid count: the kernels told the
    counts (``ref_valid``: the zero suffix is not walked) and not told (they walk the zero tiles like any other) - same output
    (tests/test_gpu_valid_refs.py).  ``expected_ratio`` = (t + valid) / (t + N): attention time in proportion to the segments."""
    from instantrestore_amd import ops as _o
    t = 1 if train_input else 0
    rows = []
    for nv in sorted({max(N // 2, 1), max(N // 4, 0), N - 1}):
        if nv >= N:
            continue
        valid = torch.full((B,), nv, dtype=torch.int32, device=dev)
        kz, vz = [k.clone() for k in keys], [v.clone() for v in vals]
        for k, v in zip(kz, vz):
            _o.zero_invalid_refs(k, v, valid, heads=k.shape[-1] // _o.HEAD_DIM)
        st = None
        if cst is not None:      # cached content statistics: an all-zero V has statistics (0, 0)
            keep = (torch.arange(N, device=dev)[None, :] < valid[:, None]).float()[:, :, None, None]
            st = [None if c is None else ((c[0] * keep).contiguous(), (c[1] * keep).contiguous()) for c in cst]
        sec_told = _time_steps(lambda: hot_path_step(layers, B, N, cached_kv=(kz, vz, st, valid)), steps)
        sec_walk = _time_steps(lambda: hot_path_step(layers, B, N, cached_kv=(kz, vz, st)), steps)
        rows.append({"valid": nv, "of": N, "ms_per_step_counts_passed": round(sec_told * 1e3, 4), "ms_per_step_zero_tiles_walked": round(sec_walk * 1e3, 4),
                     "ratio_to_all_valid": round(sec_told / sec_all_valid, 3), "expected_ratio_attention_only": round((t + nv) / (t + N), 3)})
        del kz, vz
    return {"all_valid_ms_per_step": round(sec_all_valid * 1e3, 4), "rows": rows,
            "note": "nine shared layers on cached K/V (the kv_cached leg); the projections and the self segment do not shrink with the valid count"}


def extra_probs_dump(layers, B, N, train_input, dtype, dev):
    """The dump path (attn_processors.py:258-261; what gradio_demo.py:108-109 turns on for every request): ``ir_attn_probs`` at
    the three layer classes of the config - HIP-event time per launch, GB/s of the H*L*Lkv*2 bytes it writes, and that rate as a
    fraction of the copy and fill rates measured HERE, now, on this box (a 1 GiB -> 1 GiB copy, a 1 GiB fill).  Plus the opt-in
    per-segment mass: what a consumer that only ranks the references needs, without the tensor - as a second pass
    (``ir_attn_segment_mass``) and as a by-product of the attention launch itself (ABI v9 ``seg_mass``)."""
    from instantrestore_amd import ops as _o

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    n = 1 << 29
    src = torch.empty(n, dtype=dtype, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbs = 2 * n * 2 / timed(lambda: dst.copy_(src), 5) / 1e6      # bytes read + bytes written
    fill_gbs = n * 2 / timed(lambda: dst.fill_(0.5), 5) / 1e6
    del src, dst
    t = 1 if train_input else 0
    per_class, total_ms, total_bytes = [], 0.0, 0.0
    seen = set()
    for ly in layers:
        L, C, H = ly["L"], ly["C"], ly["H"]
        if (L, C) in seen:
            continue
        seen.add((L, C))
        nbytes = float(B) * H * L * (N + t) * L * 2
        if nbytes > 24e9:
            per_class.append({"L": L, "H": H, "skipped": "%.1f GB of probabilities" % (nbytes / 1e9)})
            continue
        g = torch.Generator(device=dev).manual_seed(5)
        q, k, v = (torch.randn(B, L, C, device=dev, generator=g).to(dtype) for _ in range(3))
        rk, rv = (torch.randn(B, N, L, C, device=dev, generator=g).to(dtype) for _ in range(2))
        _, lse = _o.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=bool(t), return_lse=True)
        iters = 3 if nbytes > 2e9 else 10
        ms = timed(lambda: _o.attn_probs(q, k, rk, lse, heads=H, scale=0.125, include_self=bool(t)), iters)
        ms_old = timed(lambda: _o.attn_probs(q, k, rk, lse, heads=H, scale=0.125, include_self=bool(t), kernel="generic"), iters)
        ms_mass = timed(lambda: _o.attn_segment_mass(q, k, rk, lse, heads=H, scale=0.125, include_self=bool(t)), iters)
        # the masses as a by-product of the attention launch (ABI v9 seg_mass) against the launch alone
        ms_attn = timed(lambda: _o.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=bool(t)), 10)
        ms_attn_mass = timed(lambda: _o.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=bool(t), return_mass=True), 10)
        gbs = nbytes / ms / 1e6
        per_class.append({"L": L, "H": H, "Lkv": (N + t) * L, "gb_written": round(nbytes / 1e9, 3), "ms": round(ms, 4), "gb_per_s": round(gbs, 1),
                          "frac_of_copy_rate": round(gbs / copy_gbs, 3), "frac_of_fill_rate": round(gbs / fill_gbs, 3),
                          "ms_round1_kernel_2byte_stores": round(ms_old, 4), "ms_segment_mass_second_pass": round(ms_mass, 4),
                          "ms_attention": round(ms_attn, 4), "ms_attention_with_segment_mass_by_product": round(ms_attn_mass, 4)})
        total_ms += 3 * ms
        total_bytes += 3 * nbytes
        del q, k, v, rk, rv, lse
    return {"kernel": "attn_probs_lines_kernel (whole 128-B lines per store; segment lengths multiples of 8)",
            "copy_rate_gb_per_s_measured_here": round(copy_gbs, 1), "fill_rate_gb_per_s_measured_here": round(fill_gbs, 1),
            "layer_classes": per_class, "ms_per_step_all_nine_layers": round(total_ms, 3), "gb_per_step": round(total_bytes / 1e9, 2),
            "note": "with save_self_attentions on, every shared layer also writes its (B, H, L, Lkv) probabilities; HBM-write bound. "
                    "Not part of the headline step (inference/test.py:97 turns it on only for visualisation)"}


def extra_e2e(B, N, px, dtype, steps, dev):
    """End-to-end leg on the attention-topology host (instantrestore_amd/unet_host.py: SD-Turbo's 32 attention
    processors on both UNets with the real widths; conv/ResNet bodies, VAE and caption encoder are STAND-INS, SURVEY
    section 2 puts them out of scope), with the reference's own stage names (pix2pix_turbo.py:288-336) + the caller's
    pre/post-processing (test.py:54-59,139).  Stage times from HIP events on one stream."""
    from types import SimpleNamespace
    import __graft_entry__ as ge
    from face_replace.models.attn_processors import register_attention_processor, register_attention_processor_kv_unet
    from instantrestore_amd import ops
    from instantrestore_amd.kv_harvest import get_conditioning_keys_values
    from instantrestore_amd.preprocess import LanczosPreprocessor
    from instantrestore_amd.unet_host import AttnTopologyUNet
    sys.path.insert(0, os.path.join(REPO, "examples"))
    from synthetic_inference import StandInVAE

    cfg = SimpleNamespace(use_adain=True, train_input=True, condition_on_face_embeds=False)
    original_unet, unet = AttnTopologyUNet(seed=1).to(dev), AttnTopologyUNet(seed=2).to(dev)
    ge.register_attention_processor_kv_unet_default(original_unet, cfg)
    register_attention_processor_kv_unet(original_unet)
    register_attention_processor(unet, cfg)
    vae = StandInVAE().to(dev)
    caption = torch.randn(1, 77, 1024, device=dev)
    gen = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (px, px, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(B + B * N)]
    pre = LanczosPreprocessor(px, dtype)
    names = ["Preprocessing (uint8 -> [-1,1], device)", "VAE Encoding (stand-in)", "Get Keys and Values",
             "UNet", "Post-processing + VAE Decode (stand-in) + tensor2im"]

    def one(record=None):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        batch = pre(imgs)
        x, cond = batch[:B], batch[B:]
        ev[1].record()
        zx, zc = vae.encode(x), vae.encode(cond)
        ev[2].record()
        keys, vals, stats = get_conditioning_keys_values(original_unet, zc, None, caption.expand(B * N, -1, -1), N, [N] * B,
                                                         with_stats=True)   # one stream: AdaIN content statistics from the capture layers
        ev[3].record()
        z = unet(zx, None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": keys, "ref_values": vals, "ref_stats": stats}).sample
        ev[4].record()
        out = ops.tensor2im_u8(vae.decode(z))
        ev[5].record()
        if record is not None:
            record.append(ev)
        return out

    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        for _ in range(2):
            out = one()
        rec = []
        sec = _time_steps(lambda: one(rec), steps)
    torch.cuda.synchronize()
    stage_ms = [round(sum(e[i].elapsed_time(e[i + 1]) for e in rec) / len(rec), 3) for i in range(len(names))]
    assert out.shape == (B, px, px, 3)
    del original_unet, unet
    return {"images_per_s": round(B / sec, 2), "ms_per_batch": round(sec * 1e3, 3), "identities": B,
            "stages_ms": dict(zip(names, stage_ms)),
            "note": "attention-topology host: all 32 attention processors of both UNets at SD-Turbo widths run the HIP "
                    "path; conv/ResNet bodies, VAE and caption encoder are stand-ins (out of scope) - not end-to-end "
                    "InstantRestore throughput"}


def extra_scatter_gather(B_local, N, px, world, rank, dev, backend, single_rank_comm=None):
    """the batch scatter (degraded + references, fp16) and the output gather as grouped point-to-point
    transfers over the process group - RCCL send/recv when N > 1 - outside the headline timing."""
    from instantrestore_amd import sharding
    if os.environ.get("IR_BENCH_SG_HANG") == str(rank):   # test hook: this rank never enters the transfers
        time.sleep(1e6)
    total = B_local * world
    dt = torch.float16
    step = lambda d, r: d * 1.0    # stands for the restoration of the shard: (b,3,px,px) -> (b,3,px,px)
    if backend != "nccl" and world > 1:
        # control-flow test hook (gloo, CPU tensors): the HIP image kernels have no CPU fallback, so the transfers carry
        # pre-normalised fp16 tensors both ways (the round-2 form of this leg)
        tdev = torch.device("cpu")
        deg = torch.zeros(total, 3, px, px, dtype=dt, device=tdev) if rank == 0 else None
        refs = torch.zeros(total, N, 3, px, px, dtype=dt, device=tdev) if rank == 0 else None
        run = lambda: sharding.run_sharded(step, deg, refs, total, (3, px, px), N, dt, tdev)
        want_shape, path = (total, 3, px, px), "fp16 tensors both ways (CPU test hook)"
        nbytes = (1 + N) * 3 * px * px * 2 + 3 * px * px * 2
    else:
        # the image kernels fused with the shard buffers: raw uint8 images -> Lanczos preprocess writes
        # the identity-major send buffer -> one transfer per peer -> step -> tensor2im on every rank -> uint8 pixels back
        tdev = dev
        g = torch.Generator().manual_seed(7)
        images = [[torch.randint(0, 256, (px, px, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(1 + N)]
                  for _ in range(total)] if rank == 0 else None
        loop = bool(world == 1 and single_rank_comm and single_rank_comm.get("ok"))   # N = 1: both transfers through RCCL to this rank itself
        run = lambda: sharding.run_sharded_images(step, images, total, N, px, dt, tdev, loopback=loop)
        if loop:
            try:        # same bytes as the slicing path, or the leg says so
                a, b = run(), sharding.run_sharded_images(step, images, total, N, px, dt, tdev)
                torch.cuda.synchronize()
                single_rank_comm["loopback_equals_slicing"] = bool(torch.equal(a, b))
            except Exception as e:
                single_rank_comm.update({"ok": False, "error": "loopback send/recv: %s: %s" % (type(e).__name__, e)})
                loop = False
                run = lambda: sharding.run_sharded_images(step, images, total, N, px, dt, tdev)
        want_shape, path = (total, px, px, 3), "uint8 images in, Lanczos preprocess into the send buffers, uint8 pixels back"
        nbytes = (1 + N) * 3 * px * px * 2 + 3 * px * px
    for _ in range(2):
        run()
    if tdev.type == "cuda":
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        out = run()
    if tdev.type == "cuda":
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    ms = (time.perf_counter() - t0) / reps * 1e3
    ok = (out is not None and tuple(out.shape) == want_shape) if rank == 0 else out is None or world == 1
    one_rank = world == 1 and single_rank_comm and single_rank_comm.get("ok")
    res = {"scatter_gather_ms": round(ms, 3), "rccl_ranks": (dist.get_world_size() if (world > 1 or one_rank) else 1),
           "backend": backend if (world > 1 or one_rank) else "none (one rank: slicing only)", "path": path,
           "bytes_per_identity_on_the_links": nbytes, "ok": bool(ok)}
    if world == 1 and single_rank_comm is not None:
        res["single_rank_communicator"] = dict(single_rank_comm, note="N = 1: a real one-rank RCCL communicator; barrier, MAX reduction and "
                                               "both transfers (ncclSend + ncclRecv to this rank, one group) ran through it - no xGMI link is "
                                               "involved and NO SCALING CURVE is measured by it")
    return res


def _guarded(fn, dev, seconds):
    """Run ``fn`` - inline when ``seconds`` is None, else in a helper thread joined with a timeout.  Returns (result or
    {"error": ...}, timed_out).  A collective that never returns cannot be interrupted; the caller then skips every
    further collective and leaves through os._exit once its line is printed."""
    import threading
    box = {}

    def run():
        try:
            if dev is not None and dev.type == "cuda":
                torch.cuda.set_device(dev)
            box["r"] = fn()
        except Exception as e:
            box["r"] = {"error": "%s: %s" % (type(e).__name__, e)}

    if seconds is None:
        run()
        return box.get("r"), False
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(seconds)
    if th.is_alive():
        return {"error": "no result after %.0f s (watchdog)" % seconds}, True
    return box.get("r"), False


def init_single_rank_nccl(dev):
    """a one-rank ``nccl`` (= RCCL) process group on ``dev`` over a loopback TCP store on a free port.  Returns a report dict;
    ``ok`` False (with the error) when RCCL could not be brought up - the caller then runs without a process group."""
    import socket
    try:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        t0 = time.perf_counter()
        dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)
        x = torch.ones(1, device=dev)
        dist.all_reduce(x)          # forces the communicator into existence (lazy otherwise) and runs one RCCL kernel
        torch.cuda.synchronize()
        return {"ok": True, "backend": "nccl", "ranks": dist.get_world_size(), "init_s": round(time.perf_counter() - t0, 3)}
    except Exception as e:
        try:
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:
            pass
        return {"ok": False, "error": "%s: %s" % (type(e).__name__, e)}


def self_launch(n_gpus):
    """re-exec this script as N ranks of one node under torch.distributed.run; returns the launcher's exit code"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    log("bench.py: --gpus %d without a launcher: %s" % (n_gpus, " ".join(cmd)))
    return subprocess.run(cmd, env=env).returncode


def control_plane_only(args):
    """IR_BENCH_CONTROL_ONLY=1 (tests/test_bench_launch.py, CPU box): everything of an N-rank run that is not the GPU step -
    rendezvous, the barrier and the MAX reduction of the timed region, the scatter / gather leg of SURVEY 8e over the
    process group (gloo, CPU tensors), one JSON line from rank 0 - so that `python bench.py --gpus 2` is exercised end to end
    where there is no GPU.  `value` is null: nothing was measured."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    backend = os.environ.get("IR_BENCH_DIST_BACKEND", "gloo")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    B, N, px, _, _ = CONFIGS[args.config]
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))                          # stands for the K timed steps: rank r takes (r + 1) * 10 ms
    own = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)   # before the barrier: not the wait for the slowest rank
    if world > 1:
        dist.barrier()
    # the MAX is taken over the same per-rank times, so max_over_ranks_s and per_rank_ms_per_step agree by construction (the GPU
    # path's headline MAX is of the time bracketed by the closing barrier; the per-rank figures are own times in both)
    t = own.clone()
    per_rank_ms = [float(own.item()) * 1e3 / args.steps]
    if world > 1:
        gathered = [torch.zeros_like(own) for _ in range(world)]
        dist.all_gather(gathered, own)                     # every rank's own time beside the MAX
        per_rank_ms = [float(g.item()) * 1e3 / args.steps for g in gathered]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    # small images: control flow, not a measurement (one rank: the leg's HIP image kernels would need the GPU)
    sg = extra_scatter_gather(B, N, 64, world, rank, torch.device("cpu"), backend) if world > 1 else {"skipped": "one rank"}
    if world > 1:
        dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "restored images/sec @512px, 4 refs, single-step; 1/2/4/8 MI355X", "value": None,
                          "control_plane_only": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "max_over_ranks_s": round(float(t.item()), 4), "scaling": "weak",
                          "config": {"workload": args.config, "identities_per_gpu": B, "global_batch": B * world,
                                     "parallelism": "dp%d (independent identities)" % world,
                                     "rccl_ranks": (dist.get_world_size() if world > 1 else 1),
                                     "per_rank_ms_per_step": [round(x, 4) for x in per_rank_ms],
                                     "scatter_gather_ms": sg.get("scatter_gather_ms"), "extras": {"scatter_gather": sg}}}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def dump_outputs(outs, out_dir, budget_bytes=60 << 20, seed=0):
    """--dump-outputs: the step's nine shared-attention outputs (B, L, C) as DIR/shared_attn_out_<i>.npy, float32.  An output
    larger than its share of the budget keeps a sample of its token rows - the same sorted rows for every identity and
    channel, drawn from a generator seeded by ``seed + i`` - so that two builds are compared element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = budget_bytes // (4 * len(outs))        # float32 elements per output
    for i, o in enumerate(outs):
        o = o.detach()
        if o.numel() > share:
            rows = max(1, share // (o.numel() // o.shape[1]))
            g = torch.Generator(device="cpu").manual_seed(seed + i)
            idx = torch.randperm(o.shape[1], generator=g)[:rows].sort().values
            o = o.index_select(1, idx.to(o.device))
        np.save(os.path.join(out_dir, "shared_attn_out_%d.npy" % i), o.float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--train-input", type=int, default=1, help="1: self K/V precede the reference K/V (t=1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--variant", type=int, default=0, help="kernel variant for A/B (ir_set_attn_variant); 0 = default")
    ap.add_argument("--two-streams", type=int, default=1,
                    help="1: reference-UNet layers on their own HIP stream, shared layer i waits for capture layer i only")
    ap.add_argument("--graph", type=int, default=1,
                    help="1 (default): the timed steps REPLAY one hipGraph of the step (both streams, fork / join through the "
                         "processors' events), captured once during warm-up - same launches, same work, no CPU launch gaps; "
                         "0: eager launches (the round-1/2 headline; reported under config.extras either way)")
    ap.add_argument("--act-dtype", default="fp32", choices=["fp32", "lowp"],
                    help="fp32 (default): fp32 weights and token activations under torch.autocast, as inference/test.py:61-83 "
                         "runs the model (the 16-bit cast is part of the step); lowp: everything pre-cast to the 16-bit dtype")
    ap.add_argument("--no-extras", action="store_true", help="skip the labelled extra legs (one stream, hipGraph, cached "
                                                              "K/V, end-to-end host, scatter/gather)")
    ap.add_argument("--ref-early-exit", action="store_true",
                    help="stop the reference UNet after the K/V projections of its last capturing layer (its output is "
                         "discarded by the inference caller); off for the headline number")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: the roofline and per-kernel-class figures, the "
                         "CPU baseline, the labelled extra legs (one stream, second graph capture, cached K/V, power, probs dump, "
                         "cfg1gpu, end-to-end host, scatter / gather) and, at N = 1, the one-rank RCCL communicator.  Off "
                         "(default): set up, warm up, time the K steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the nine shared-attention outputs of the last timed step to "
                         "DIR/shared_attn_out_<i>.npy (float32; a fixed, seeded sample of token rows where an output is large)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    # what only --full runs; the --no-* switches still narrow a --full run
    no_roofline = args.no_roofline or not args.full
    no_cpu_baseline = args.no_cpu_baseline or not args.full
    no_extras = args.no_extras or not args.full

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own (the shape of the driver's N = 1 command): become the launcher - one rank per
        # GPU under torch.distributed.run on this node, rendezvous on 127.0.0.1 - and hand its exit code back.  The
        # torchrun form (`python -m torch.distributed.run ... bench.py --gpus N`) keeps working: it sets WORLD_SIZE.
        sys.exit(self_launch(args.gpus))
    if os.environ.get("IR_BENCH_CONTROL_ONLY") == "1":
        sys.exit(control_plane_only(args))

    # the result line is the only thing on stdout: what libraries print there through C stdio (librccl announces its versions)
    # goes to stderr, and the line is written to a duplicate of the original descriptor
    sys.stdout.flush()
    line_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the hot path)")
    # test hooks (tests/test_bench_contract.py drives the N = 2 control flow on a one-GPU box): every rank on
    # cuda:0 and the two control-plane collectives (barrier, MAX of the elapsed time) over gloo
    backend = os.environ.get("IR_BENCH_DIST_BACKEND", "nccl")
    dev_index = 0 if os.environ.get("IR_BENCH_SHARE_DEVICE") == "1" else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    single_rank_comm = None   # world == 1: {"backend": "nccl", ...} once a REAL one-rank RCCL communicator exists, else why not
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            # RCCL over xGMI.  A communicator that does not come up must not hang the node for torch's default ten minutes:
            # the bring-up (and every collective after it) gives up after IR_BENCH_RCCL_TIMEOUT seconds and the run fails loudly
            import datetime
            dist.init_process_group(backend="nccl", device_id=dev,
                                    timeout=datetime.timedelta(seconds=float(os.environ.get("IR_BENCH_RCCL_TIMEOUT", "300"))))
        else:
            dist.init_process_group(backend=backend)
    elif args.full and os.environ.get("IR_BENCH_FORCE_DIST", "1") == "1" and backend == "nccl":
        # N = 1 (round 5): the barrier, the MAX-over-ranks reduction and the scatter / gather leg run through
        # a real one-rank RCCL communicator, so that the first 8-GPU run is not also the first RCCL run.  Never at the price of
        # the headline: any failure falls back to the plain single-process path and is reported in extras.scatter_gather.
        #   ... and never at the price of the run either: the bring-up happens under a watchdog (a communicator that never
        #   comes up must not keep the headline from being measured); a stuck helper thread is left behind and the process leaves
        #   through os._exit once its line is printed
        single_rank_comm, init_hung = _guarded(lambda: init_single_rank_nccl(dev), dev, float(os.environ.get("IR_BENCH_RCCL_INIT_TIMEOUT", "90")))
        if init_hung or not isinstance(single_rank_comm, dict) or "ok" not in single_rank_comm:
            single_rank_comm = {"ok": False, "error": (single_rank_comm or {}).get("error", "one-rank RCCL bring-up failed"), "init_hung": bool(init_hung)}
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    use_dist = world > 1 or (single_rank_comm is not None and single_rank_comm.get("ok"))
    leave_hard = bool(single_rank_comm and single_rank_comm.get("init_hung"))

    train_input = bool(args.train_input)
    if args.variant:
        from instantrestore_amd import ops as _ops
        _ops.set_attn_variant(args.variant)
    act_fp32 = args.act_dtype == "fp32"
    layers, (B, N, px, dtype, use_adain) = build_workload(args.config, train_input, dev, seed=1234 + rank, act_fp32=act_fp32)
    _AUTOCAST["dtype"] = dtype if act_fp32 else None

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    cap, launch_mode, graph_error = None, "eager launches", None
    with torch.no_grad():
        for _ in range(args.warmup):
            outs = hot_path_step(layers, B, N, args.ref_early_exit, bool(args.two_streams))
        if args.graph and not args.ref_early_exit:
            # the step captured ONCE (untimed, part of the warm-up); every timed step is one replay of that graph
            try:
                cap = CapturedStep(layers, B, N, bool(args.two_streams))
                for _ in range(max(2, args.warmup)):     # untimed: the replayed step warmed up like the eager one
                    cap.replay()
                launch_mode = "hipGraph replay (one capture during warm-up)"
            except Exception as e:      # capture is an optimisation: the eager step is always there
                cap, graph_error = None, "%s: %s" % (type(e).__name__, e)
        barrier()
        # HIP events on the launch stream around the dominant kernel's launches INSIDE the timed region
        # (the shared attention of the largest layer class: 3 launches per step) - eager launches only: inside a graph
        # replay there is no launch to bracket, the in-step figure then comes from an eager run after the timing
        from instantrestore_amd import ops as _ops_mod
        top_l = layers[-1]["L"]
        in_step = []
        if rank == 0 and not no_roofline and cap is None:
            _ops_mod.EVENT_SINK = (lambda q, rk, ad: rk is not None and q.shape[1] == top_l, in_step)
        t0 = time.perf_counter()
        if cap is not None:
            for _ in range(args.steps):
                cap.replay()
            outs = cap.outs
        else:
            for _ in range(args.steps):
                outs = hot_path_step(layers, B, N, args.ref_early_exit, bool(args.two_streams))
        torch.cuda.synchronize()
        own = time.perf_counter() - t0      # this rank's own K steps, before it waits for the other ranks at the barrier
        barrier()   # synchronize + barrier + synchronize: the K steps are bracketed on both sides
        elapsed = time.perf_counter() - t0
        _ops_mod.EVENT_SINK = None
        if rank == 0 and args.dump_outputs:     # before anything else runs on the layers: the last timed step's results
            dump_outputs(outs, args.dump_outputs)
        if rank == 0 and not no_roofline and cap is not None and args.two_streams:
            _ops_mod.EVENT_SINK = (lambda q, rk, ad: rk is not None and q.shape[1] == top_l, in_step)
            for _ in range(args.steps):
                hot_path_step(layers, B, N, False, True)
            torch.cuda.synchronize()
            _ops_mod.EVENT_SINK = None
        in_step_ms = [a.elapsed_time(b) for a, b in in_step]
    assert all(torch.isfinite(o).all() for o in outs)
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    per_rank_ms = [own / args.steps * 1e3]
    if use_dist:
        own_t = torch.tensor([own], dtype=torch.float64, device=t.device)
        gathered = [torch.zeros_like(own_t) for _ in range(dist.get_world_size())]
        dist.all_gather(gathered, own_t)        # every rank's own time for its K steps (the line reports them beside the MAX)
        per_rank_ms = [float(g.item()) / args.steps * 1e3 for g in gathered]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    roof = cpu = None
    if rank == 0:
        if not no_roofline:
            # `achieved`: the dominant kernel's average launch duration INSIDE timed steps, HIP events on its
            # launch stream - over a second timed region of the same K steps run on ONE stream, because with two
            # streams the reference UNet's kernels share the chip with it and the in-situ time stops being the
            # kernel's own.  The back-to-back figure (20 launches on an idle GPU, measured afterwards) is kept
            # next to it: a sustained run of this one kernel clocks lower than the same kernel between the
            # step's lighter kernels.
            one_stream = []
            _ops_mod.EVENT_SINK = (lambda q, rk, ad: rk is not None and q.shape[1] == top_l, one_stream)
            with torch.no_grad():
                for _ in range(args.steps):
                    hot_path_step(layers, B, N, args.ref_early_exit, False)
            torch.cuda.synchronize()
            _ops_mod.EVENT_SINK = None
            roof = measure_roofline(layers, B, N, train_input, use_adain, dtype)
            b2b = {k: roof[k] for k in ("achieved", "frac", "ms_per_launch")}
            ms_in = sum(a.elapsed_time(b) for a, b in one_stream) / len(one_stream)
            tf_in = roof["algorithmic_gflop_per_launch"] / ms_in
            roof.update({"achieved": round(tf_in, 2), "frac": round(tf_in / roof["peak"], 4), "ms_per_launch": round(ms_in, 4),
                         "launches_timed": len(one_stream),
                         "timing": "HIP events on the launch stream around every launch of this kernel inside K timed steps (one stream)",
                         "back_to_back": b2b})
            if in_step_ms and args.two_streams:
                ms2 = sum(in_step_ms) / len(in_step_ms)
                roof["in_step_two_streams"] = {"ms_per_launch": round(ms2, 4), "launches": len(in_step_ms),
                                               "note": "in the headline run: includes time shared with the other stream's kernels"}
            # the WHOLE step against the same peak: algorithmic attention flops of all 18 layers / the headline step time
            from instantrestore_amd.roofline import summary as _summary
            sm = _summary(N, train_input, px)
            step_tflop = B * (sm["shared_gflop_per_identity"] + sm["kv_capture_gflop_per_identity"]) / 1e3
            step_ms = elapsed / args.steps * 1e3
            roof["step"] = {"attention_tflop_per_step": round(step_tflop, 4), "achieved": round(step_tflop / step_ms * 1e3, 2),
                            "frac": round(step_tflop / step_ms * 1e3 / roof["peak"], 4), "unit": "TFLOP/s",
                            "note": "attention flops of the 9 capture + 9 shared layers / ms_per_step of the headline run; the "
                                    "projections, AdaIN statistics and launch gaps are in the time and not in the flops",
                            "kernel_classes_one_stream": kernel_class_breakdown(layers, B, N, max(2, args.steps // 2))}
        if world == 1 and roof is not None and os.environ.get("IR_BENCH_LIVE_PMC") == "1" and roof.get("traffic") is not None:
            live, detail = live_pmc_traffic()
            roof["traffic_committed_pass"] = roof["traffic"]
            if live is not None:
                roof["traffic"], roof["traffic_static"], roof["traffic_live_detail"] = live, False, detail
                roof["traffic_unit"] = "bytes/launch (PMC in THIS run: 2*FETCH_SIZE + WRITE_SIZE, two counter-only rocprofv3 passes of tools/prof_attn.py)"
            else:
                roof["traffic_live_error"] = detail
        if world == 1 and not no_cpu_baseline:
            cpu = cpu_baseline(N, px, train_input, use_adain, seed=99, dtype=dtype, dev=dev)
    extras = None
    hung = False
    if not no_extras:
        extras = {}
        if rank == 0:
            with torch.no_grad():
                sec1 = _time_steps(lambda: hot_path_step(layers, B, N, args.ref_early_exit, False), args.steps)
                extras["one_stream"] = {"images_per_s": round(B / sec1, 2), "ms_per_step": round(sec1 * 1e3, 4),
                                        "note": "same step, eager launches, both UNets on one HIP stream (the reference's own schedule)"}
                sec2 = _time_steps(lambda: hot_path_step(layers, B, N, args.ref_early_exit, True), args.steps)
                extras["eager_two_streams"] = {"images_per_s": round(B / sec2, 2), "ms_per_step": round(sec2 * 1e3, 4),
                                               "note": "same step, eager launches on two HIP streams (the headline of rounds 1-2)"}
                try:
                    secg, same, gdetail = extra_graph(layers, B, N, args.steps)
                    extras["hip_graph"] = {"images_per_s": round(B / secg, 2), "ms_per_step": round(secg * 1e3, 4),
                                           "bit_identical_to_eager": bool(same), "compared": gdetail,
                                           "note": "a SECOND capture of the two-stream step, replayed and compared tensor by tensor "
                                                   "(9 outputs + 18 harvested K/V) with a fresh eager run"}
                except Exception as e:   # capture is an extra: never lose the headline over it
                    extras["hip_graph"] = {"error": "%s: %s" % (type(e).__name__, e)}
                keys, vals, cst = [], [], []
                for ly in layers:   # resident reference K/V (+ AdaIN content statistics) of the batch's identities: what ReferenceKVCache.assemble returns
                    ly["kv_attn"].processor.capture_stats = bool(use_adain)
                    with torch.autocast("cuda", dtype=dtype):
                        ly["kv_attn"](ly["h_ref"])
                    p = ly["kv_attn"].processor
                    keys.append(p.keys.reshape(-1, N, *p.keys.shape[1:]).clone())
                    vals.append(p.values.reshape(-1, N, *p.values.shape[1:]).clone())
                    if p.v_part is not None:
                        cst.append(_ops_mod.RefStatsPartials(p.v_part, p.values.shape[0] // N, N, p.values.shape[1]).finished())
                    else:
                        cst.append(None if p.v_mean is None else (p.v_mean.reshape(-1, N, *p.v_mean.shape[-2:]).clone(), p.v_std.reshape(-1, N, *p.v_std.shape[-2:]).clone()))
                    p.reset()
                secc = _time_steps(lambda: hot_path_step(layers, B, N, cached_kv=(keys, vals, cst if use_adain else None)), args.steps)
                extras["kv_cached"] = {"images_per_s": round(B / secc, 2), "ms_per_step": round(secc * 1e3, 4),
                                       "note": "reference K/V served from the per-identity cache (SURVEY 8f rank 2): only the nine "
                                               "shared layers run; valid when the references of an identity repeat across frames"}
                try:
                    extras["ragged_valid"] = extra_ragged_valid(layers, B, N, keys, vals, cst if use_adain else None, secc, train_input, args.steps, dev)
                except Exception as e:
                    extras["ragged_valid"] = {"error": "%s: %s" % (type(e).__name__, e)}
                del keys, vals, cst
                try:
                    pstep = cap.replay if cap is not None else (lambda: hot_path_step(layers, B, N, args.ref_early_exit, bool(args.two_streams)))
                    extras["power"] = power_probe(pstep, float(os.environ.get("IR_BENCH_POWER_SECONDS", "3")))
                except Exception as e:
                    extras["power"] = {"error": "%s: %s" % (type(e).__name__, e)}
                try:
                    extras["probs_dump"] = extra_probs_dump(layers, B, N, train_input, dtype, dev)
                except Exception as e:
                    extras["probs_dump"] = {"error": "%s: %s" % (type(e).__name__, e)}
                if args.config == "cfg2":
                    try:
                        extras["cfg1gpu"] = extra_cfg1gpu(dev, max(10, args.steps), act_fp32)
                    except Exception as e:
                        extras["cfg1gpu"] = {"error": "%s: %s" % (type(e).__name__, e)}
                if args.config != "cfg5":
                    try:
                        extras["e2e_topology_host"] = extra_e2e(B, N, px, dtype, max(2, args.steps // 2), dev)
                    except Exception as e:
                        extras["e2e_topology_host"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # The collective extra must never cost the headline (measured above): with N > 1 it runs under a watchdog - a rank
        # that fails or stalls inside RCCL would otherwise leave the others waiting in their transfers for ever
        if world > 1:   # rank 0 has just run the single-rank extras: the others wait for it HERE, not inside the timed extra
            _, hung = _guarded(lambda: dist.barrier(), dev, 900.0)
        if hung:
            sg = {"error": "skipped: the ranks did not meet at the barrier before it"}
        else:
            sg, hung = _guarded(lambda: extra_scatter_gather(B, N, px, world, rank, dev, backend, single_rank_comm), dev,
                                float(os.environ.get("IR_BENCH_SG_TIMEOUT", "120")) if (world > 1 or use_dist) else None)
        extras["scatter_gather"] = sg
    if world > 1 and not hung:
        _, hung = _guarded(lambda: dist.barrier(), dev, 60.0)

    if rank == 0:
        from instantrestore_amd.roofline import summary
        ms = elapsed / args.steps * 1e3
        total_ids = B * world
        pw = (extras or {}).get("power") or {}
        if roof and pw.get("sclk_mhz_avg"):
            # informational: `peak` / `frac` above stay the guide's 2.4 GHz figures; this is the same ratio at the clock the
            # power cap left the step (rocm-smi average over the sustained run of extras.power)
            pk = roof["peak"] * pw["sclk_mhz_avg"] / pw["sclk_peak_mhz"]
            roof["at_measured_clock"] = {"sclk_mhz": pw["sclk_mhz_avg"], "watts": pw["watts_avg"], "peak_at_clock": round(pk, 1),
                                         "frac_at_clock": round(roof["achieved"] / pk, 4),
                                         "note": "step-average clock under the 1400 W cap; not the contract's frac"}
        if roof:
            # what the matrix pipe itself sustains on THIS box under the board's power cap, measured now (ir_bench_mfma_stream: an
            # MFMA-only stream of the kernel's instruction, ~0.15 s per setting): the contract's `peak` is the 2.4 GHz figure,
            # which random operands never see.  Informational: `frac` stays achieved / peak.
            try:
                from instantrestore_amd import ops as _o
                cap_r = _o.bench_mfma_stream(dtype, zero_operands=False, device=dev)
                cap_z = _o.bench_mfma_stream(dtype, zero_operands=True, device=dev)
                roof["at_power_cap"] = {"mfma_only_tflops_random_operands": round(cap_r, 1), "mfma_only_tflops_zero_operands": round(cap_z, 1),
                                        "frac_of_sustained": round(roof["achieved"] / cap_r, 4),
                                        "note": "MFMA-only stream of v_mfma_f32_32x32x16 (two waves per SIMD, every CU) measured in this run; "
                                                "on random operands the 1400 W cap sets it, on zeros the clock does; not the contract's frac"}
            except Exception as e:   # a measurement aid must not cost the line
                roof["at_power_cap"] = {"error": "%s: %s" % (type(e).__name__, e)}
        line = {
            "metric": "restored images/sec @512px, 4 refs, single-step; 1/2/4/8 MI355X",
            "metric_note": "one step = one pass of the HOT PATH only (attention path of both UNets, SURVEY 8a a-1..a-4): "
                           "identities pushed through it per second, NOT end-to-end restoration throughput (conv/ResNet/VAE "
                           "stages are out of scope and not in the step); %s, %s" % (launch_mode, "two HIP streams" if args.two_streams else "one HIP stream"),
            "value": round(total_ids / (elapsed / args.steps), 3),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype],
            "data": "synthetic",
            "config": {
                "workload": "%s: hot path only (SURVEY 8a a-1..a-4) = 9 K/V-capture layers over B*N reference token "
                            "sets + harvest + 9 shared-attention layers (to_q/k/v, AdaIN stats, fused extended "
                            "attention, to_out) over B identities; UNet conv/ResNet and VAE stages are out of scope "
                            "and not in the step" % args.config,
                "identities_per_gpu": B, "global_batch": total_ids, "refs": N, "px": px,
                "use_adain": use_adain, "train_input": train_input, "ref_early_exit": bool(args.ref_early_exit), "two_streams": bool(args.two_streams), "launch": launch_mode, "graph_capture_error": graph_error, "parallelism": "dp%d (independent identities)" % world,
                "activations": "fp32 under torch.autocast (test.py:61-83)" if act_fp32 else "pre-cast to the 16-bit dtype",
                "layer_dependence": "none: the nine layer pairs of the synthetic step are independent token sets (the UNet body that would chain them "
                                    "is out of scope), so a replayed graph / two streams may overlap ANY of them; in the real UNet layer i+1 waits for "
                                    "layer i of its own UNet and only the two UNets overlap (the one-stream figure under extras is the no-overlap bound)",
                "rccl_ranks": (dist.get_world_size() if use_dist else 1),
                "per_rank_ms_per_step": [round(x, 4) for x in per_rank_ms],
                "rccl_communicator": ("real (%d ranks)" % dist.get_world_size()) if use_dist else "none: %s" % ((single_rank_comm or {}).get("error") or ("IR_BENCH_FORCE_DIST=0" if args.full else "one rank, no --full")),
                "scatter_gather_ms": None if not extras else extras.get("scatter_gather", {}).get("scatter_gather_ms"),
                "extras": extras,
                **{k: round(v, 1) for k, v in summary(N, train_input, px).items()},
            },
            "roofline": roof,
            "cpu_baseline": cpu,
        }
        print(json.dumps(line), file=line_out, flush=True)
    if leave_hard:      # a helper thread is still inside the RCCL bring-up: no interpreter teardown behind it
        sys.stdout.flush()
        os._exit(0)
    if world == 1 and use_dist:
        if hung:
            os._exit(0)
        try:
            dist.destroy_process_group()
        except Exception:
            pass
    if world > 1:
        if hung:   # some rank is stuck in a collective: the line is out, leave without the teardown that would wait for it
            sys.stdout.flush()
            sys.stderr.write("bench.py: rank %d leaves without process-group teardown (collective extra timed out)\n" % rank)
            sys.stderr.flush()
            os._exit(0)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
