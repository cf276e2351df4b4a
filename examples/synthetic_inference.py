#!/usr/bin/env python3
"""The call pattern of ``face_replace/inference/test.py:79-187`` end to end on the MI355X path, with
synthetic weights (no checkpoint is reachable offline) and stand-ins for the stages that are out of
scope (VAE, UNet conv/ResNet body, caption encoder):

    uint8 images (any sizes)                        -> LanczosPreprocessor      (test.py:54-59, on the device)
    references  -> stand-in VAE encode -> frozen reference UNet on a side stream, early exit after the last
                   K/V capture                      -> get_conditioning_keys_values / harvest (pix2pix_turbo.py:242-279)
    degraded    -> stand-in VAE encode -> main UNet, 9 shared-attention layers waiting on per-layer events
                                                    -> SharedAttnProcessor      (attn_processors.py:193-279)
    result      -> stand-in VAE decode              -> tensor2im_u8             (vis_utils.py:14-23, on the device)

    python examples/synthetic_inference.py [--identities 2] [--refs 4] [--px 512] [--dtype fp16]
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class StandInVAE(nn.Module):
    """8x average pooling + 1x1 projection to 4 latent channels, and its inverse: only there so tensors of
    the right shapes flow between the stages this repository implements"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.enc = nn.Parameter(torch.randn(4, 3, generator=g) * 0.5, requires_grad=False)
        self.dec = nn.Parameter(torch.randn(3, 4, generator=g) * 0.5, requires_grad=False)

    def encode(self, x):                       # (B,3,S,S) -> (B,4,S/8,S/8)
        return torch.einsum("oc,bchw->bohw", self.enc.to(x.dtype), nn.functional.avg_pool2d(x, 8))

    def decode(self, z):                       # (B,4,s,s) -> (B,3,8s,8s) in [-1,1]
        y = torch.einsum("oc,bchw->bohw", self.dec.to(z.dtype), z)
        return torch.tanh(nn.functional.interpolate(y, scale_factor=8, mode="nearest"))


MUTUAL_MIN_FACTOR = 2.0     # --mutual: a reference token is kept when some query token gives it this many times the uniform probability 1 / Lkv


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--identities", type=int, default=2)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--px", type=int, default=512)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--small", action="store_true", help="narrow UNet topology (tests)")
    ap.add_argument("--landmark-maps", action="store_true",
                    help="one more frame that leaves the landmark attention map of every shared layer behind (attention_rows)")
    ap.add_argument("--matches", action="store_true",
                    help="one more frame that leaves the best-matching token of every reference behind for every query token "
                         "(attention_match): prints, per shared layer, the mean best probability per reference and where the best matches lie")
    ap.add_argument("--topk", type=int, default=None, metavar="K",
                    help="one more frame that leaves the K best tokens of every reference behind for every query token (attention_topk, "
                         "K = 1 ... 8): prints, per shared layer and reference, the mean ambiguity (runner-up / best, the ratio test) and the "
                         "mean share of the reference's attention its K best keys carry")
    ap.add_argument("--prune-topk", action="store_true",
                    help="with --topk: prints the fraction of reference tokens that are among the K best of any query token "
                         "(attn_maps.keep_from_topk, a keep mask for ops.compact_refs)")
    ap.add_argument("--transfer", action="store_true",
                    help="one more frame that leaves the attention-weighted mean position inside every reference behind for every query "
                         "token (attention_transfer with the coordinate payload): prints, per shared layer and reference, the mean soft "
                         "displacement, the mean mass and how often the rounded expected position is attention_match's hard match")
    ap.add_argument("--mutual", action="store_true",
                    help="one more frame that leaves, beside attention_match, the best query token of every key behind (attention_key_match): "
                         "prints, per shared layer and reference, the share of query tokens whose match survives the mutual check "
                         "(attn_maps.mutual_matches) and the share of reference tokens attn_maps.keep_from_key_match keeps at one threshold")
    ap.add_argument("--received", action="store_true",
                    help="one more frame that leaves, for every token of every reference, the attention it receives from the whole "
                         "degraded face behind (attention_received, unweighted): prints, per shared layer, the received mass per reference")
    ap.add_argument("--prune", type=float, default=None, metavar="FRACTION",
                    help="with --received: keep that fraction of every reference's tokens, the ones the top shared layer looked at most on "
                         "the warm-up frame (attn_maps.keep_from_received -> ops.compact_refs -> ref_lens); prints the top layer's masses "
                         "and the kept counts with and without")
    ap.add_argument("--ref-weights", default=None,
                    help="comma-separated weight per reference, e.g. 1,1,0.25,0 (0 masks a reference): prints the top shared layer's "
                         "per-reference attention masses with and without")
    ap.add_argument("--compact-refs", type=float, default=None, metavar="FRACTION",
                    help="keep a centred elliptical region of that area of every reference (e.g. 0.5): the kept tokens are packed to the "
                         "front of their segments once (ops.compact_refs) and the shared layers walk the counts (ref_lens); prints the top "
                         "shared layer's attention masses with and without")
    ap.add_argument("--adain-keep", type=float, default=None, metavar="FRACTION",
                    help="mask-aware AdaIN (adain_weights): the statistics behind the affine are taken over a centred elliptical region of "
                         "that area of every reference and of the image alone; prints the largest change of the affine (a, b) and of the "
                         "output against the unmasked run.  With --compact-refs the packed references carry kept-token statistics "
                         "(ops.token_stats_weighted(packed_v, lens=lens)) instead of those of the full references")
    ap.add_argument("--adain-regions", type=int, default=None, metavar="R",
                    help="per-region AdaIN (adain_regions / adain_n_regions): a synthetic parsing map of R classes (1 ... 32; horizontal bands, "
                         "shifted by one band on every further reference); every shared layer renormalises a reference token with the "
                         "statistics of ITS class on both sides.  Prints how far the affine table's regional slots lie from the whole-face "
                         "affine and the largest change of the output against plain AdaIN")
    ap.add_argument("--regions", action="store_true",
                    help="one more cached frame under a per-query restriction by region labels (region_labels / region_allow): synthetic label "
                         "pictures - a 4 x 4 grid of classes, shifted by n cells on reference n - and the rule \"own class only, self "
                         "free\"; prints the top shared layer's attention masses with and without")
    ap.add_argument("--kv-tables", action="store_true",
                    help="one more cached frame whose reference K/V are pointer tables into the cache entries (assemble_tables: no copy)")
    args = ap.parse_args(argv)
    if args.prune is not None and not args.received:
        ap.error("--prune chooses its tokens from the attention they received: give --received with it")
    if args.prune_topk and args.topk is None:
        ap.error("--prune-topk chooses its tokens from the K best keys: give --topk K with it")

    import __graft_entry__ as ge
    from face_replace.models.attn_processors import register_attention_processor, register_attention_processor_kv_unet
    from instantrestore_amd import ops
    from instantrestore_amd.kv_cache import ReferenceKVCache
    from instantrestore_amd.kv_harvest import enable_ref_stats, enable_stream_overlap, finished_stats, harvest_reference_kv
    from instantrestore_amd.attn_processors import ReferenceCaptureComplete, AttnProcessor
    from instantrestore_amd.preprocess import LanczosPreprocessor
    from instantrestore_amd.unet_host import AttnTopologyUNet

    dev = torch.device("cuda", 0)
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    B, N, S = args.identities, args.refs, args.px
    cfg = SimpleNamespace(use_adain=True, train_input=True, condition_on_face_embeds=False)
    topo = dict(block_out_channels=(64, 128, 128, 128), attention_head_dim=(1, 2, 2, 2), cross_attention_dim=64) if args.small else {}
    cross = topo.get("cross_attention_dim", 1024)
    original_unet, unet = AttnTopologyUNet(seed=1, **topo).to(dev), AttnTopologyUNet(seed=2, **topo).to(dev)
    ge.register_attention_processor_kv_unet_default(original_unet, cfg)
    register_attention_processor_kv_unet(original_unet)
    register_attention_processor(unet, cfg)
    enable_stream_overlap(original_unet)
    enable_ref_stats(original_unet)        # the capture layers also stash the AdaIN content statistics of every reference V
    vae = StandInVAE().to(dev)
    caption = torch.randn(1, 77, cross, device=dev)          # fixed caption embedding (pix2pix_turbo.py:100-106)

    # raw uint8 images of assorted sizes, as a decoder would leave them in HBM
    gen = torch.Generator().manual_seed(0)
    sizes = [(S, S), (S + S // 2, S), (S, 2 * S), (700, 933), (1024, 1024)]
    mk = lambda i: torch.randint(0, 256, (*sizes[i % len(sizes)], 3), generator=gen, dtype=torch.uint8).to(dev)
    degraded_u8 = [mk(i) for i in range(B)]
    refs_u8 = [mk(B + i) for i in range(B * N)]

    pre = LanczosPreprocessor(S, dtype)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        batch = pre(degraded_u8 + refs_u8)                    # (B + B*N, 3, S, S) in [-1, 1]
        x, cond = batch[:B], batch[B:]
        # reference branch on the side stream, stopping after the last K/V capture
        side.wait_stream(torch.cuda.current_stream())
        procs = [p for p in original_unet.attn_processors.values() if type(p) in [AttnProcessor]]
        for p in procs:
            p.reset()
            p.stop_after_capture = procs
        with torch.cuda.stream(side):
            try:
                original_unet(vae.encode(cond), None, encoder_hidden_states=caption.expand(B * N, -1, -1))
            except ReferenceCaptureComplete:
                pass
        for p in procs:
            p.stop_after_capture = None
        keys, values, events, stats = harvest_reference_kv(original_unet, N, [N] * B, with_events=True, with_stats=True)
        # main branch: every shared layer waits for its own reference layer only
        z = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": keys, "ref_values": values, "ref_events": events, "ref_stats": stats}).sample
        torch.cuda.current_stream().wait_stream(side)
        out_u8 = ops.tensor2im_u8(vae.decode(z))              # (B, S, S, 3) uint8
        # NEXT FRAME of the same identities: the references have not changed, so neither have their K/V nor their AdaIN
        # content statistics - both come out of the per-identity cache and the whole reference branch is skipped
        cache = ReferenceKVCache(max_identities=max(8, B))
        stats = finished_stats(stats)                         # (mean, std) pairs: sliceable per identity
        for b in range(B):
            cache.get_or_compute("id%d" % b, lambda b=b: ([k[b:b + 1] for k in keys], [v[b:b + 1] for v in values],
                                                          [(m[b:b + 1], sd[b:b + 1]) for m, sd in stats]))
        ck, cv, cs = cache.assemble(["id%d" % b for b in range(B)])
        z2 = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                  cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs}).sample
        assert torch.equal(ops.tensor2im_u8(vae.decode(z2)), out_u8), "cached K/V + statistics must reproduce the frame"
        if args.kv_tables:
            # the same cached frame without the (B, N, L, C) copies of assemble(): every layer gets a table of pointers into the
            # per-identity entries (one small host-to-device copy for all 18 tables), and the kernels read the entries in place
            tk, tv, ts, tvalid = cache.assemble_tables(["id%d" % b for b in range(B)])
            z3 = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                      cross_attention_kwargs={"ref_keys": tk, "ref_values": tv, "ref_stats": ts, "ref_valid": tvalid}).sample
            assert torch.equal(ops.tensor2im_u8(vae.decode(z3)), out_u8), "pointer tables into the cache must reproduce the frame"
        # A checkpoint trained with fewer references than the caller hands in (inference/test.py:81 passes ITS
        # max_conditioning_images as valid count; pix2pix_turbo.py:269-273 zero-fills the rest): told the counts
        # (cross_attention_kwargs['ref_valid'], what harvest_reference_kv(..., with_valid=True) returns) the kernels close the
        # zeroed references analytically instead of walking them - same pixels.  And a consumer that only ranks the references
        # (gradio_demo.py:119-127) asks the top shared layer for its per-reference attention mass instead of attention_probs.
        if N > 1:
            valid = torch.full((B,), N - 1, dtype=torch.int32, device=dev)
            zk, zv = [k.clone() for k in ck], [v.clone() for v in cv]
            for k, v in zip(zk, zv):
                ops.zero_invalid_refs(k, v, valid, heads=k.shape[-1] // 64)
            top = [p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) == 8][0]
            top.save_attention_mass = True
            kw = {"ref_keys": zk, "ref_values": zv}          # (no cached statistics here: the zero fill changed them)
            z3 = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1), cross_attention_kwargs=dict(kw, ref_valid=valid)).sample
            mass = top.attention_mass                          # (B, H, L, 1 + N) fp32, rows sum to 1
            z4 = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1), cross_attention_kwargs=kw).sample
            top.save_attention_mass = False
            assert float((z3.float() - z4.float()).abs().max()) <= 2e-2 * max(1.0, float(z4.float().abs().max()))
            assert mass.shape[-1] == N + int(top.train_input) and float((mass.sum(-1) - 1).abs().max()) < 2e-3
        # "Trust photo 2 less, ignore photo 3": per-reference weights ride into the fused kernel as an additive key bias (log w on a
        # reference's keys; 0 masks it - no attention at all, unlike a zero-filled reference); the masses are the read-back
        if args.ref_weights:
            w = torch.tensor([float(t) for t in args.ref_weights.split(",")], device=dev)
            assert w.numel() == N and bool((w >= 0).all()), f"--ref-weights needs {N} values >= 0"
            top = [p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) == 8][0]
            top.save_attention_mass = True
            kw = {"ref_keys": keys, "ref_values": vals}
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1), cross_attention_kwargs=kw)
            m0 = top.attention_mass.mean(dim=(1, 2))
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs=dict(kw, ref_weights=w.expand(B, N).contiguous()))
            m1 = top.attention_mass.mean(dim=(1, 2))
            top.save_attention_mass = False
            fmt = lambda m: " ".join(f"{v:.3f}" for v in m.tolist())
            for b in range(B):
                print(f"identity {b}: mass [self?] ++ references  unweighted {fmt(m0[b])}  |  weights {args.ref_weights}: {fmt(m1[b])}")
            assert all(float(m1[:, int(top.train_input) + n].abs().max()) == 0.0 for n in range(N) if float(w[n]) == 0.0)
        # "Only the face region of every reference": a keep map is turned into FEWER KEYS, once per identity - the kept tokens of a
        # reference packed to the front of its segment, per-reference counts for the shared layers (ref_lens) - instead of a mask
        # that every frame pays for (ref_token_keep: the key bias walks every tile).  The AdaIN statistics stay those of the full
        # references (cs, taken before compaction), as with a mask.
        if args.compact_refs is not None:
            import math
            frac = float(args.compact_refs)
            assert 0.0 < frac <= 1.0, "--compact-refs needs a fraction in (0, 1]"
            a = 64 * math.sqrt(frac / (1.25 * math.pi))                     # a centred ellipse, axes 1 : 1.25, on a 64 x 64 map
            yy, xx = torch.meshgrid(torch.arange(64) + 0.5 - 32, torch.arange(64) + 0.5 - 32, indexing="ij")
            keep = ((xx / a) ** 2 + (yy / (1.25 * a)) ** 2 <= 1.0).to(dev).expand(B, N, 64, 64)
            packed = [ops.compact_refs(k, v, keep, heads=k.shape[-1] // 64) for k, v in zip(ck, cv)]     # pooled to every layer's side
            top = [p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) == 8][0]
            top.save_attention_mass = True
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            m0 = top.attention_mass.mean(dim=(1, 2))
            zc = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                      cross_attention_kwargs={"ref_keys": [t[0] for t in packed], "ref_values": [t[1] for t in packed], "ref_stats": cs,
                                              "ref_lens": [t[2] for t in packed]}).sample
            m1 = top.attention_mass.mean(dim=(1, 2))
            top.save_attention_mass = False
            fmt = lambda m: " ".join(f"{v:.3f}" for v in m.tolist())
            kept = packed[8][2][0].tolist()
            for b in range(B):
                print(f"identity {b}: mass [self?] ++ references  full {fmt(m0[b])}  |  {kept} of {ck[8].shape[2]} tokens kept: {fmt(m1[b])}")
            assert bool(torch.isfinite(zc).all()) and float((m1.sum(-1) - 1).abs().max()) < 2e-3
        # "Renormalise the face with the FACE's statistics": the AdaIN affine comes from the statistics over the tokens of a centred
        # region of the image and of every reference alone (adain_weights: a weight picture per side, sampled by every shared layer
        # at its own token centres) - the background no longer pollutes mean and std.  The affine is an input of the attention,
        # so this composes with the compacted references above: their statistics are then taken over the packed rows.
        if args.adain_keep is not None:
            import math
            frac = float(args.adain_keep)
            assert 0.0 < frac <= 1.0, "--adain-keep needs a fraction in (0, 1]"
            a = 64 * math.sqrt(frac / (1.25 * math.pi))
            yy, xx = torch.meshgrid(torch.arange(64) + 0.5 - 32, torch.arange(64) + 0.5 - 32, indexing="ij")
            region = ((xx / a) ** 2 + (yy / (1.25 * a)) ** 2 <= 1.0).to(dev)
            self_w, ref_w = region.expand(B, 64, 64).contiguous(), region.expand(B, N, 64, 64).contiguous()
            affines, real = [], ops.shared_attention

            def recording(*a_, **kw_):          # the affine every shared layer hands the attention, in layer order
                if kw_.get("adain") is not None:
                    affines.append(kw_["adain"])
                return real(*a_, **kw_)
            ops.shared_attention = recording
            try:
                kw = {"ref_keys": ck, "ref_values": cv, "ref_stats": cs}
                z0 = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1), cross_attention_kwargs=kw).sample
                plain, affines = affines, []
                zm = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                          cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "adain_weights": (self_w, ref_w)}).sample
                masked, affines = affines, []
                da = max(float((m[0] - p[0]).abs().max()) for m, p in zip(masked, plain))
                db = max(float((m[1] - p[1]).abs().max()) for m, p in zip(masked, plain))
                print(f"--adain-keep {frac}: {int(region.sum())} of 4096 map pixels kept; largest change of a {da:.3f}, of b {db:.3f}, of the "
                      f"output {float((zm.float() - z0.float()).abs().max()):.3f} (max|output| {float(z0.float().abs().max()):.3f})")
                assert bool(torch.isfinite(zm).all()) and len(masked) == len(plain) == 9
                if args.compact_refs is not None:
                    # the compacted call of --compact-refs with kept-token statistics: one counted pass over the packed V per layer
                    kept_stats = [ops.token_stats_weighted(t[1], heads=t[1].shape[-1] // 64, lens=t[2]) for t in packed]
                    zk = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                              cross_attention_kwargs={"ref_keys": [t[0] for t in packed], "ref_values": [t[1] for t in packed],
                                                      "ref_stats": kept_stats, "ref_lens": [t[2] for t in packed],
                                                      "adain_weights": (self_w, None)}).sample
                    print(f"  with --compact-refs {args.compact_refs}: kept-token statistics of the packed references; largest change of the "
                          f"output against the compacted call with full-reference statistics {float((zk.float() - zc.float()).abs().max()):.3f}")
                    assert bool(torch.isfinite(zk).all())
            finally:
                ops.shared_attention = real
        # "Renormalise eye tokens with eye statistics, skin with skin": one affine per (reference, class) instead of one per reference.
        # A parsing map per side goes in once (the one region_labels takes); every shared layer samples it at its own token centres,
        # takes the statistics of every class in one pass over V (ops.token_stats_regions), builds the (B, N, R + 1, H, 64) table
        # (ops.adain_affine_regions: a class too small on either side falls back to the whole-face affine) and forms the renormalised
        # V once (ops.adain_apply_regions); the attention then runs without an affine.
        if args.adain_regions is not None:
            R, px = int(args.adain_regions), 64
            assert 1 <= R <= 32, "--adain-regions needs 1 ... 32 classes"
            band = (torch.arange(px, device=dev) * R // px)[:, None].expand(px, px)            # (px, px): class = horizontal band
            q_labels = band.expand(B, px, px).contiguous()
            ref_labels = torch.stack([torch.roll(band, shifts=n * max(1, px // R), dims=0) for n in range(N)]).expand(B, N, px, px).contiguous()
            tables, real = [], ops.adain_affine_regions

            def recording(*a_, **kw_):          # the table every shared layer builds, in layer order
                tables.append(real(*a_, **kw_))
                return tables[-1]
            ops.adain_affine_regions = recording
            try:
                kw = {"ref_keys": ck, "ref_values": cv, "ref_stats": cs}
                z0 = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1), cross_attention_kwargs=kw).sample
                zr = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                          cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "adain_regions": (q_labels, ref_labels),
                                                  "adain_n_regions": R}).sample
            finally:
                ops.adain_affine_regions = real
            da = max(float((a_[:, :, :R] - a_[:, :, R:]).abs().max()) for a_, _ in tables)
            db = max(float((b_[:, :, :R] - b_[:, :, R:]).abs().max()) for _, b_ in tables)
            regional = sum(int(((a_[:, :, :R] != a_[:, :, R:]).flatten(3).any(-1)).sum()) for a_, _ in tables)
            print(f"--adain-regions {R}: {len(tables)} shared layers, {regional} of {sum(a_[:, :, :R, 0, 0].numel() for a_, _ in tables)} "
                  f"(reference, class) slots carry regional statistics; largest distance of a regional slot from the whole-face affine: a {da:.3f}, "
                  f"b {db:.3f}; largest change of the output {float((zr.float() - z0.float()).abs().max()):.3f} "
                  f"(max|output| {float(z0.float().abs().max()):.3f})")
            assert bool(torch.isfinite(zr).all()) and len(tables) == 9
        # "Eye tokens draw from eye tokens of the references, mouth from mouth, the picture itself is free": a per-QUERY restriction.
        # Label pictures (a face parsing map; here a coarse grid of classes) and a class-by-class rule go in once; every shared layer
        # samples the labels at its own token centres and hands the kernel one 32-bit word per query row and one small integer per
        # key (ops.region_masks) - never a (Lq, Lkv) mask.  AdaIN is unchanged; the masses are the read-back.
        if args.regions:
            G, px = 4, 64
            cell = torch.arange(px, device=dev) * G // px
            grid = cell[:, None] * G + cell[None, :]                                       # (px, px): classes 0 .. G * G - 1
            q_labels = grid.expand(B, px, px).contiguous()
            ref_labels = torch.stack([torch.roll(grid, shifts=n * (px // G), dims=1) for n in range(N)]).expand(B, N, px, px).contiguous()
            allow = torch.eye(G * G, dtype=torch.bool, device=dev)                        # own class only
            top = [p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) == 8][0]
            top.save_attention_mass = True
            kw = {"ref_keys": ck, "ref_values": cv, "ref_stats": cs}
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1), cross_attention_kwargs=kw)
            m0 = top.attention_mass.mean(dim=(1, 2))
            zr = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                      cross_attention_kwargs=dict(kw, region_labels=(q_labels, ref_labels), region_allow=allow)).sample
            m1 = top.attention_mass.mean(dim=(1, 2))
            top.save_attention_mass = False
            fmt = lambda m: " ".join(f"{v:.3f}" for v in m.tolist())
            for b in range(B):
                print(f"identity {b}: mass [self?] ++ references  unrestricted {fmt(m0[b])}  |  {G * G} classes, own class only, self free: {fmt(m1[b])}")
            assert bool(torch.isfinite(zr).all()) and float((m1.sum(-1) - 1).abs().max()) < 2e-3
        # Where do the facial landmarks look (vis_utils.py:88-110)?  Each shared layer is told which query tokens they fall on
        # and leaves the sum of those tokens' head-mean probability rows behind - (B, Lkv) fp32, reshaped to one side x 5*side
        # picture over the degraded image and its references - instead of the (B, H, L, Lkv) tensor of save_self_attentions.
        if args.landmark_maps:
            import numpy as np
            from instantrestore_amd.attn_maps import landmark_picture, landmark_rows
            landmarks = np.random.default_rng(0).uniform(0.2 * 512, 0.8 * 512, size=(68, 2))       # 68 seeded pseudo-landmarks, (x, y) at 512 px
            shared = sorted((p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) is not None),
                            key=lambda p: p.self_attn_idx)
            side_of = {}
            for p in shared:
                tokens = keys[p.self_attn_idx].shape[2]
                if tokens < len(landmarks):        # a toy resolution: ir_attn_rows takes at most len_q rows (the model's smallest shared layer has 256 tokens)
                    continue
                side_of[p.self_attn_idx] = int(round(tokens ** 0.5))
                p.attention_rows_index = torch.from_numpy(landmark_rows(landmarks, side_of[p.self_attn_idx]))
                p.attention_rows_reduce = "map"
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            for p in shared:
                if p.self_attn_idx not in side_of:
                    continue
                m, p.attention_rows_index = p.attention_rows, None
                pic = landmark_picture(m[0], side_of[p.self_attn_idx])
                print(f"shared layer {p.self_attn_idx}: landmark map {tuple(m.shape)} fp32, sum per identity {[round(float(t), 3) for t in m.sum(-1)]} "
                      f"(68 rows of probabilities), picture {pic.shape}")
                assert float((m.sum(-1) - 68).abs().max()) < 68 * 8e-3
        # Which token of each reference does every token of the degraded face draw from, and how strongly?  Each shared layer
        # leaves (index, prob) of the head-mean attention behind - int32 / fp32 (B, L, [self?] + N): the best key of every segment
        # and its probability - instead of the (B, H, L, Lkv) tensor; attn_maps.match_coordinates turns the indices into (y, x).
        if args.matches:
            from instantrestore_amd.attn_maps import match_coordinates
            shared = sorted((p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) is not None),
                            key=lambda p: p.self_attn_idx)
            for p in shared:
                p.attention_match_index = "all"
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            fmt = lambda m: " ".join(f"{v:.4f}" for v in m.tolist())
            for p in shared:
                (index, prob), p.attention_match_index = p.attention_match, None
                first = int(p.train_input)                                       # column of reference 0
                rp, ri = prob[..., first:], index[..., first:]                   # (B, L, N)
                tokens = ck[p.self_attn_idx].shape[2]
                share = torch.bincount(rp.argmax(-1).flatten(), minlength=N).float() / rp[..., 0].numel()
                side_len = int(round(tokens ** 0.5))
                y, xq = match_coordinates(ri, side_len)
                print(f"shared layer {p.self_attn_idx}: match {tuple(index.shape)}; mean best probability per reference {fmt(rp.mean(dim=(0, 1)))}; "
                      f"share of tokens whose best match lies in each reference {fmt(share)}")
                assert int(ri.min()) >= 0 and int(ri.max()) < tokens and int(y.max()) < side_len and 0 <= int(xq.min()) and int(xq.max()) < side_len
                assert float(prob.min()) > 0 and float(prob.sum(-1).max()) <= 1.0 + 8e-3 and abs(float(share.sum()) - 1) < 1e-5
        # One best key cannot tell one sharp peak from two equal ones (two eyes, two brows, rows of teeth).  Each shared layer leaves
        # (index, prob) of the K best keys of every segment behind - int32 / fp32 (B, L, [self?] + N, K), rank 0 being the match
        # above - and the segment masses of the same launch say how much of a reference's attention those K keys carry.
        if args.topk is not None:
            from instantrestore_amd.attn_maps import keep_from_topk, match_ambiguity, topk_coverage
            K = int(args.topk)
            shared = sorted((p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) is not None),
                            key=lambda p: p.self_attn_idx)
            for p in shared:
                p.attention_topk_index, p.attention_topk_k, p.save_attention_mass = "all", K, True
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            fmt = lambda m: " ".join(f"{v:.4f}" for v in m.tolist())
            for p in shared:
                (index, prob), p.attention_topk_index = p.attention_topk, None
                mass, p.save_attention_mass = p.attention_mass.mean(dim=1), False       # (B, L, S): of the head mean
                first = int(p.train_input)                                       # column of reference 0
                tokens = ck[p.self_attn_idx].shape[2]
                cover = topk_coverage(prob, mass)[..., first:]                   # (B, L, N)
                line = f"shared layer {p.self_attn_idx}: top-{K} {tuple(index.shape)}"
                if K >= 2:
                    line += f"; mean ambiguity per reference {fmt(match_ambiguity(prob)[..., first:].mean(dim=(0, 1)))}"
                line += f"; mean coverage of the {K} best keys per reference {fmt(cover.mean(dim=(0, 1)))}"
                if args.prune_topk:
                    keep = keep_from_topk(index, N, tokens, bool(p.train_input))     # (B, N, tokens) bool
                    line += f"; fraction of reference tokens keep_from_topk keeps {float(keep.float().mean()):.4f}"
                    assert keep.shape == (B, N, tokens) and bool(keep.any(-1).all())
                print(line)
                assert int(index[..., :min(K, tokens)].min()) >= 0 and int(index.max()) < tokens
                assert float(cover.min()) > 0 and float(cover.max()) <= 1 and bool((prob[..., :-1] >= prob[..., 1:]).all())
        # Every query token has a best key in every reference - occluded skin, hair and background too, where it is the best of a bad
        # lot.  The mutual (cycle) check keeps the pair (token i, key j) only if j is the best key of i AND i is the best token of
        # j: each shared layer leaves the best query token of every key behind (attention_key_match, the column maximum of the
        # attention without the (B, H, L, Lkv) tensor) beside attention_match of the same frame.  The column maximum itself is a keep
        # rule for reference tokens: those that at least one query token looks at with MUTUAL_MIN_FACTOR times the uniform
        # probability 1 / Lkv or more.
        if args.mutual:
            from instantrestore_amd.attn_maps import keep_from_key_match, mutual_matches
            shared = sorted((p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) is not None),
                            key=lambda p: p.self_attn_idx)
            for p in shared:
                p.attention_match_index, p.attention_match_reduce, p.attention_key_match_reduce = "all", "head_mean", "head_mean"
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            fmt = lambda m: " ".join(f"{v:.4f}" for v in m.tolist())
            for p in shared:
                (index, _), p.attention_match_index = p.attention_match, None
                (key_index, key_prob), p.attention_key_match_reduce = p.attention_key_match, None
                first = int(p.train_input)                                       # column of reference 0
                tokens = ck[p.self_attn_idx].shape[2]
                mutual = mutual_matches(index, key_index, tokens, N, tokens, bool(p.train_input))       # (B, L, S) bool
                min_prob = MUTUAL_MIN_FACTOR / key_prob.shape[-1]
                keep = keep_from_key_match(key_prob, tokens, N, tokens, bool(p.train_input), min_prob=min_prob)
                print(f"shared layer {p.self_attn_idx}: key match {tuple(key_index.shape)}; share of query tokens whose match survives the "
                      f"mutual check per reference {fmt(mutual[..., first:].float().mean(dim=(0, 1)))}; share of reference tokens some "
                      f"query token looks at with p >= {min_prob:.2e} {fmt(keep.float().mean(dim=(0, 2)))}")
                assert mutual.shape == index.shape and keep.shape == (B, N, tokens)
                assert int(key_index.min()) >= 0 and int(key_index.max()) < index.shape[1] and float(key_prob.min()) >= 0
                # a key has ONE best token: at most one surviving pair per key
                assert int(mutual[..., first:].sum(dim=1).max()) <= tokens
        # Where in each reference does every token of the degraded face look, to a fraction of a token?  The payload holds the
        # (y, x) of every key; each shared layer leaves (sums, mass) of the head-mean attention behind - fp32 (B, L, [self?] + N, 2)
        # and (B, L, [self?] + N) - and soft_match_field divides: the expected position inside every segment, its displacement
        # from the token's own place and the segment's mass as the confidence.  attention_match of the same frame is the hard form.
        if args.transfer:
            from instantrestore_amd.attn_maps import coordinate_payload, match_coordinates, soft_match_field
            shared = sorted((p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) is not None),
                            key=lambda p: p.self_attn_idx)
            for p in shared:
                tokens = ck[p.self_attn_idx].shape[2]
                p.attention_transfer_payload = coordinate_payload(tokens, N, tokens, bool(p.train_input), device=dev)
                p.attention_match_index = "all"
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            fmt = lambda m: " ".join(f"{v:.4f}" for v in m.tolist())
            for p in shared:
                (sums, mass), p.attention_transfer_payload = p.attention_transfer, None
                (index, _), p.attention_match_index = p.attention_match, None
                first = int(p.train_input)                                       # column of reference 0
                side_len = int(round(ck[p.self_attn_idx].shape[2] ** 0.5))
                pos, disp, conf = soft_match_field(sums, mass, "all", side_len)
                pos, disp, conf = pos[:, :, first:], disp[:, :, first:], conf[:, :, first:]      # (B, L, N, 2), (B, L, N)
                hy, hx = match_coordinates(index[..., first:], side_len)
                agree = ((pos[..., 0].round().long() == hy) & (pos[..., 1].round().long() == hx)).float().mean(dim=(0, 1))
                print(f"shared layer {p.self_attn_idx}: transfer {tuple(sums.shape)}; mean soft displacement per reference "
                      f"{fmt(disp.norm(dim=-1).mean(dim=(0, 1)))}; mean mass per reference {fmt(conf.mean(dim=(0, 1)))}; "
                      f"share of tokens whose rounded expected position is the hard match {fmt(agree)}")
                assert float(pos.min()) >= 0 and float(pos.max()) <= side_len - 1 + 1e-3 and float(mass.min()) > 0
                assert float((mass.sum(-1) - 1).abs().max()) < 8e-3
        # Which tokens of each reference does the restored face USE, and how much?  The column sums of the attention: each shared
        # layer leaves fp32 (B, Lkv, 1) behind - per key, the head-mean attention summed over every query token - instead of the
        # (B, H, L, Lkv) tensor.  A reference's received mass is its share of the L units the query tokens hand out.  With --prune
        # that warm-up frame decides which tokens every later frame of the identity keeps: data-driven, where --compact-refs
        # keeps a centred ellipse.
        if args.received:
            from instantrestore_amd.attn_maps import keep_from_received, received_maps
            shared = sorted((p for p in unet.attn_processors.values() if getattr(p, "self_attn_idx", None) is not None),
                            key=lambda p: p.self_attn_idx)
            for p in shared:
                p.attention_received_weights = "ones"
            unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                 cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
            fmt = lambda m: " ".join(f"{v:.4f}" for v in m.tolist())
            recv_top = None
            for p in shared:
                recv, p.attention_received_weights = p.attention_received, None
                tokens = ck[p.self_attn_idx].shape[2]
                maps = received_maps(recv, tokens, N, tokens, bool(p.train_input))         # (B, S, side, side, 1)
                per_seg = maps.sum(dim=(2, 3, 4)) / tokens                                  # (B, S): shares of the query tokens' attention
                print(f"shared layer {p.self_attn_idx}: received {tuple(recv.shape)}; received mass [self?] ++ references "
                      f"{fmt(per_seg.mean(dim=0))}; largest share of one token {float(recv.max()) / tokens:.4f}")
                assert float(recv.min()) >= 0 and float((per_seg.sum(-1) - 1).abs().max()) < 8e-3
                if p.self_attn_idx == 8:
                    recv_top = recv
            if args.prune is not None:
                frac = float(args.prune)
                assert 0.0 < frac <= 1.0, "--prune needs a fraction in (0, 1]"
                top = [p for p in shared if p.self_attn_idx == 8][0]
                tokens = ck[8].shape[2]
                side_len = int(round(tokens ** 0.5))
                keep = keep_from_received(recv_top, tokens, N, tokens, bool(top.train_input), frac)       # (B, N, tokens) bool
                packed = [ops.compact_refs(k, v, keep.view(B, N, side_len, side_len), heads=k.shape[-1] // 64)
                          for k, v in zip(ck, cv)]                                                    # pooled to every layer's side
                top.save_attention_mass = True
                unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                     cross_attention_kwargs={"ref_keys": ck, "ref_values": cv, "ref_stats": cs})
                m0 = top.attention_mass.mean(dim=(1, 2))
                zp = unet(vae.encode(x), None, encoder_hidden_states=caption.expand(B, -1, -1),
                          cross_attention_kwargs={"ref_keys": [t[0] for t in packed], "ref_values": [t[1] for t in packed], "ref_stats": cs,
                                                  "ref_lens": [t[2] for t in packed]}).sample
                m1 = top.attention_mass.mean(dim=(1, 2))
                top.save_attention_mass = False
                fmt3 = lambda m: " ".join(f"{v:.3f}" for v in m.tolist())
                for b in range(B):
                    print(f"identity {b}: mass [self?] ++ references  full {fmt3(m0[b])}  |  pruned to {packed[8][2][b].tolist()} of {tokens} "
                          f"tokens by received attention: {fmt3(m1[b])}")
                assert bool(torch.isfinite(zp).all()) and float((m1.sum(-1) - 1).abs().max()) < 2e-3
                assert packed[8][2].tolist() == [[int(keep[b, n].sum()) for n in range(N)] for b in range(B)]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out_u8.shape == (B, S, S, 3) and out_u8.dtype == torch.uint8
    assert len(keys) == 9 and keys[0].shape[:2] == (B, N)
    print(f"restored {B} synthetic identities x {N} references at {S}px in {dt*1e3:.1f} ms (first call, includes "
          f"table/plan/weight caches); output {tuple(out_u8.shape)} uint8, mean {out_u8.float().mean().item():.1f}")
    return out_u8


if __name__ == "__main__":
    main()
