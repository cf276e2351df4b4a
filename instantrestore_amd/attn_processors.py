"""Attention processors of InstantRestore, MI355X-native.

Drop-in for ``face_replace/models/attn_processors.py`` of the reference: the same six public
names, constructor signatures, ``forward`` signatures, attribute protocol
(``self_attn_idx``, ``save_self_attentions``, ``attention_probs``, ``keys``/``values``/
``reset()``) and registration functions.  The projections (``to_q/k/v``,
``to_out``) stay ``nn.Linear`` calls on the host ``attn`` object exactly as in the reference -
so peft/LoRA wrappers and autocast keep working - while everything between them, which the
reference spells as head-split copies + ``adain`` + ``cat`` + ``baddbmm``/``softmax``/``bmm``
(attn_processors.py:232-264), is ONE fused HIP kernel plus a one-pass statistics kernel
(``instantrestore_amd.ops`` -> ``include/instantrestore_hip.h``).

``attn.upcast_attention`` / ``attn.upcast_softmax`` (diffusers ``Attention``; the reference honours them through
``get_attention_scores``, attn_processors.py:257): the fused kernel ALWAYS forms the scores from the 16-bit q / k with
fp32 accumulation (products of 16-bit values are exact in fp32: the same numbers as an fp32 ``baddbmm`` of the upcast
operands) and keeps the softmax in fp32 - both flags are satisfied by construction, set or not; with them unset the
reference's own path rounds the scores to 16 bit before its softmax, which this path never does.
``tests/test_golden_r4.py`` holds both settings to the reference's outputs.

The processors own no parameters and no buffers (the reference's checkpoints are loaded with
``strict=True``, test.py:47-50).  They never fall back to torch math: CPU tensors, fp32
activations outside autocast, per-query attention masks and missing libraries raise.  A per-key ``attention_mask`` (and the
``ref_weights`` / ``ref_token_keep`` kwargs of the shared layers) becomes the fused kernel's additive key bias (``_mask_bias``).

Batch-invariant mode (ABI v10; :func:`set_batch_invariant`, or the plain attribute ``batch_invariant`` of
:class:`SharedAttnProcessor` / :class:`AttnProcessor`): every GEMM, statistics pass and attention of a processor then runs
the library's batch-invariant plans, so an identity's outputs (``attention_mass`` / ``attention_probs`` included) do not
depend on how many identities share its batch or where it sits.  A projection that would run on the vendor GEMM - a shape this
library's GEMMs do not cover, or one left to the module call (biased / unfoldable projections, autograd enabled) - raises instead.  The UNet body around the processors (convolutions, norms) is not covered.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import torch
from torch import nn

from . import lora_fold as _lora
from .ops import RefKVTable as _RefKVTable
from . import ops as _ops  # tests swap this module-level name for an oracle-backed stand-in


# ------------------------------------------------------------------------------------------
# adain(): attn_processors.py:7-18
# ------------------------------------------------------------------------------------------
def adain(content_features: torch.Tensor, style_mean: torch.Tensor, style_std: torch.Tensor) -> torch.Tensor:
    """Renormalise ``content_features`` (BH, L, 64) to the given style statistics.

    Same contract as the reference function: statistics over the token axis (dim=1), unbiased
    std, ``1e-5`` added to the content std here (the caller has already added it to
    ``style_std``, attn_processors.py:245).  The reduction and the application are HIP kernels;
    only the (BH, 1, 64)-sized algebra that turns four statistics into an affine is torch.
    """
    if content_features.dim() != 3 or content_features.shape[-1] != _ops.HEAD_DIM:
        raise ValueError("adain expects head-split features of shape (B*H, L, 64)")
    bh, length, d = content_features.shape
    x = content_features.reshape(bh, 1, length, d)
    mean, std = _ops.token_stats(x, heads=1)                      # (BH,1,1,64) fp32
    a = style_std.reshape(bh, 1, 1, d).float() / (std + _ops.ADAIN_EPS)
    b = style_mean.reshape(bh, 1, 1, d).float() - mean * a
    return _ops.adain_apply(x, a.contiguous(), b.contiguous(), heads=1).reshape(bh, length, d)


# ------------------------------------------------------------------------------------------
# shared prologue / epilogue of every processor (attn_processors.py:42-70, 84-97)
# ------------------------------------------------------------------------------------------
class _Prepared:
    __slots__ = ("hidden", "encoder", "residual", "ndim", "shape4", "mask")


def _prologue(attn, hidden_states, encoder_hidden_states, attention_mask, temb) -> _Prepared:
    st = _Prepared()
    st.residual = hidden_states
    if attn.spatial_norm is not None:
        hidden_states = attn.spatial_norm(hidden_states, temb)
    st.ndim = hidden_states.ndim
    st.shape4 = None
    if st.ndim == 4:
        st.shape4 = hidden_states.shape
        bsz, ch, hh, ww = st.shape4
        hidden_states = hidden_states.view(bsz, ch, hh * ww).transpose(1, 2)
    # an attention mask becomes the fused kernel's additive key bias (_mask_bias, once the processor knows its key axis).  The
    # host's prepare_attention_mask is not called: its target length is the self / encoder length, and a shared layer's mask
    # runs over the extended key axis
    st.mask = attention_mask
    if attn.group_norm is not None:
        hidden_states = attn.group_norm(hidden_states.transpose(1, 2)).transpose(1, 2)
    st.hidden = hidden_states
    st.encoder = encoder_hidden_states
    return st


def _mask_bias(mask, batch: int, heads: int, lkv: int, len_self: int, shared: bool) -> Optional[torch.Tensor]:
    """``attention_mask`` as the additive fp32 key bias of ``ops.shared_attention``: ``(B, Lkv)``, ``(B, 1, Lkv)`` (what diffusers'
    UNet hands the cross-attention layers for padded text, a bias of -10000) or ``(B * H, 1, Lkv)`` (the same after
    ``prepare_attention_mask``'s ``repeat_interleave`` over heads).  The reference adds it to the scaled scores
    (``get_attention_scores``: ``baddbmm`` with ``beta = 1``); here it rides into the kernel, nothing is added on the host."""
    if mask is None:
        return None
    if mask.dtype == torch.bool or not mask.is_floating_point():
        raise ValueError(f"attention_mask must be additive (floating point: 0 keeps, -10000 / -inf masks), got {mask.dtype}")
    if mask.dim() == 3:
        if mask.shape[1] != 1:
            raise NotImplementedError(f"attention_mask {tuple(mask.shape)}: a query axis of {mask.shape[1]} - per-query masks are not supported "
                                      "(the fused kernel takes one bias per key; a per-query restriction by region labels goes in as region_labels / region_allow)")
        mask = mask[:, 0]
    elif mask.dim() != 2:
        raise ValueError(f"attention_mask must be (B, Lkv), (B, 1, Lkv) or (B * H, 1, Lkv), got {tuple(mask.shape)}")
    if mask.shape[-1] != lkv:
        if shared and mask.shape[-1] == len_self:
            raise ValueError(f"attention_mask covers {len_self} keys, the self length, but this shared layer attends over {lkv} keys "
                             "([self] ++ references): pass a mask of the extended length (the reference itself would fail in baddbmm here)")
        raise ValueError(f"attention_mask covers {mask.shape[-1]} keys, the layer attends over {lkv}")
    mask = mask.to(torch.float32)
    if mask.shape[0] == batch:
        return mask
    if mask.shape[0] != batch * heads:
        raise ValueError(f"attention_mask has {mask.shape[0]} rows for a batch of {batch} with {heads} heads")
    mask = mask.view(batch, heads, lkv)
    # identical per-head rows collapse to one shared row only where that is known without a device sync (an expanded view)
    return mask[:, 0] if mask.stride(1) == 0 else mask


class _IdentityCache(dict):
    """what a shared layer builds from caller tensors, kept per (identity and version of every source, geometry): the nine shared
    layers of a step have three geometries, so they build three values.  An in-place change of a source bumps its version; a
    reused ``id`` is caught by the ``is`` check on the hit.  Bounded: the oldest entry leaves first."""

    def __init__(self, limit: int):
        super().__init__()
        self.limit = limit

    def cached(self, sources: tuple, geometry: tuple, build):
        """the value of ``build()`` for these ``sources`` (any may be ``None``) on this ``geometry``"""
        key = tuple(None if t is None else (id(t), getattr(t, "_version", None)) for t in sources) + geometry
        hit = self.get(key)
        if hit is not None and all(a is b for a, b in zip(hit[0], sources)):
            return hit[1]
        value = build()
        while len(self) >= self.limit:
            self.pop(next(iter(self)))
        self[key] = (sources, value)
        return value


_BIAS_ROWS_MAX = _REGION_PAIRS_MAX = _ADAIN_WEIGHTS_MAX = _ADAIN_REGION_LABELS_MAX = 8
_BIAS_ROWS = _IdentityCache(_BIAS_ROWS_MAX)                         # bias rows of ``ref_weights`` / ``ref_token_keep``
_REGION_PAIRS = _IdentityCache(_REGION_PAIRS_MAX)                   # (q_allow, key_region) of ``region_labels`` / ``region_allow``
_ADAIN_WEIGHTS = _IdentityCache(_ADAIN_WEIGHTS_MAX)                 # (self weights, reference weights) of ``adain_weights``
_ADAIN_REGION_LABELS = _IdentityCache(_ADAIN_REGION_LABELS_MAX)     # (self labels, reference labels) of ``adain_regions``: int32 rows

_GRID_DTYPE = {"region_labels": None, "adain_weights": torch.float32, "adain_regions": torch.int32}


def _on_grid(values, length: int, refs: bool, device, kwarg: str):
    """a picture ``(B, [N,] Hpx, Wpx)`` or per-token values ``(B, [N,] L)`` (the row-major picture of their own square grid) of
    ``kwarg``, sampled at the token centres of the square grid of ``length`` tokens, on ``device``:

    ``region_labels``: integer labels (``attn_maps.token_labels``) in their own dtype, ``(B, [N *] length)`` - the key axis lays the
    references end to end; ``length`` must be a square up front and per-token labels always pass through their own grid.
    ``adain_weights``: float or bool weights (``attn_maps.token_weights``) -> fp32 ``(B, [N,] length)``.  ``adain_regions``: integer
    labels -> int32 ``(B, [N,] length)``.  Both take per-token values of exactly ``length`` as they are, square or not."""
    from . import attn_maps as _maps
    packed, weights, dtype = kwarg == "region_labels", kwarg == "adain_weights", _GRID_DTYPE[kwarg]
    what = f"{kwarg}: the {'reference' if refs else 'self' if weights else 'query'} {'weights' if weights else 'labels'}"
    len_name = what if not packed else "len_ref" if refs else "len_q"
    side = _maps._square_side(length, len_name) if packed else None
    t = torch.as_tensor(values)
    pictures = 4 if refs else 3
    if t.dim() == pictures - 1:      # per-token values
        if not packed and t.shape[-1] == length:
            return t.to(device=device, dtype=dtype).contiguous()
        s = _maps._square_side(t.shape[-1], f"{len_name}: the per-token labels' length" if packed else f"{what}' length")
        t = t.reshape(*t.shape[:-1], s, s)
    if t.dim() != pictures:
        raise ValueError(f"{what} must be {'a weight picture' if weights else 'label pictures'} {'(B, N, Hpx, Wpx)' if refs else '(B, Hpx, Wpx)'} "
                         f"or per-token {'weights' if weights else 'labels'}, got {tuple(torch.as_tensor(values).shape)}")
    picked = (_maps.token_weights if weights else _maps.token_labels)(t, side or _maps._square_side(length, len_name))
    if not packed:
        picked = picked.reshape(*t.shape[:-2], length)
    return picked.to(device=device, dtype=dtype).contiguous()


def _ref_bias_row(ref_weights, ref_token_keep, batch: int, len_self: int, n_refs: int, len_ref: int, include_self: bool, device):
    if ref_weights is None and ref_token_keep is None:
        return None
    return _BIAS_ROWS.cached((ref_weights, ref_token_keep), (batch, len_self, n_refs, len_ref, include_self, str(device)),
                             lambda: _ops.key_bias(batch, len_self, n_refs, len_ref, include_self, ref_weights=ref_weights,
                                                   ref_token_keep=ref_token_keep, device=device))


def _region_pair(region_labels, region_allow, batch: int, len_q: int, len_self: int, n_refs: int, len_ref: int,
                 include_self: bool, device):
    if not isinstance(region_labels, (tuple, list)) or len(region_labels) != 2:
        raise ValueError("region_labels must be the pair (query_labels, ref_labels)")
    if region_allow is None:
        raise ValueError("region_labels needs region_allow: the (C, C) bool matrix or the (C,) bitmasks of ops.region_masks")
    q_lab, r_lab = region_labels

    def build():
        ql = _on_grid(q_lab, len_q, False, device, "region_labels")
        rl = _on_grid(r_lab, len_ref, True, device, "region_labels")
        if ql.shape[0] != batch or rl.shape[0] != batch or rl.shape[1] != n_refs * len_ref:
            raise ValueError(f"region_labels: labels of {tuple(ql.shape)} query and {tuple(rl.shape)} reference tokens for a batch of {batch} with "
                             f"{n_refs} references of {len_ref} tokens")
        parts = [rl.to(torch.int64)]
        if include_self:     # the self keys are this picture's own tokens: the query labels on the self grid
            parts.insert(0, (ql if len_self == len_q else _on_grid(q_lab, len_self, False, device, "region_labels")).to(torch.int64))
        return _ops.region_masks(ql, torch.cat(parts, dim=1), torch.as_tensor(region_allow).to(device),
                                 self_len=len_self if include_self else 0, self_free=True)    # a token always sees its own picture

    return _REGION_PAIRS.cached((q_lab, r_lab, region_allow), (batch, len_q, len_self, n_refs, len_ref, include_self, str(device)), build)


def _adain_weight_pair(adain_weights, batch: int, len_self: int, n_refs: int, len_ref: int, device):
    if not isinstance(adain_weights, (tuple, list)) or len(adain_weights) != 2:
        raise ValueError("adain_weights must be the pair (self_weights, ref_weights); either may be None")
    self_w, ref_w = adain_weights

    def build():
        sw = None if self_w is None else _on_grid(self_w, len_self, False, device, "adain_weights")
        rw = None if ref_w is None else _on_grid(ref_w, len_ref, True, device, "adain_weights")
        if sw is not None and tuple(sw.shape) != (batch, len_self):
            raise ValueError(f"adain_weights: self weights of {tuple(sw.shape)} tokens for a batch of {batch} with {len_self} tokens")
        if rw is not None and tuple(rw.shape) != (batch, n_refs, len_ref):
            raise ValueError(f"adain_weights: reference weights of {tuple(rw.shape)} tokens for a batch of {batch} with {n_refs} references "
                             f"of {len_ref} tokens")
        return sw, rw

    return _ADAIN_WEIGHTS.cached((self_w, ref_w), (batch, len_self, n_refs, len_ref, str(device)), build)


def _adain_region_labels(adain_regions, batch: int, len_self: int, n_refs: int, len_ref: int, device):
    if not isinstance(adain_regions, (tuple, list)) or len(adain_regions) != 2 or adain_regions[0] is None or adain_regions[1] is None:
        raise ValueError("adain_regions must be the pair (query_labels, ref_labels)")
    q_lab, r_lab = adain_regions

    def build():
        ql = _on_grid(q_lab, len_self, False, device, "adain_regions")
        rl = _on_grid(r_lab, len_ref, True, device, "adain_regions")
        if tuple(ql.shape) != (batch, len_self) or tuple(rl.shape) != (batch, n_refs, len_ref):
            raise ValueError(f"adain_regions: labels of {tuple(ql.shape)} query and {tuple(rl.shape)} reference tokens for a batch of {batch} "
                             f"with {len_self} tokens and {n_refs} references of {len_ref} tokens")
        return ql, rl

    return _ADAIN_REGION_LABELS.cached((q_lab, r_lab), (batch, len_self, n_refs, len_ref, str(device)), build)


def _kv_source(attn, st: _Prepared) -> torch.Tensor:
    if st.encoder is None:
        return st.hidden
    if attn.norm_cross:
        return attn.norm_encoder_hidden_states(st.encoder)
    return st.encoder


def _epilogue(attn, st: _Prepared, tokens: torch.Tensor, bi: bool = False) -> torch.Tensor:
    out = _project_out(attn, tokens, bi)   # linear proj (LoRA-wrapped on the main UNet)
    out = attn.to_out[1](out)      # dropout (p = 0)
    if st.ndim == 4:
        bsz, ch, hh, ww = st.shape4
        out = out.transpose(-1, -2).reshape(bsz, ch, hh, ww)
    if attn.residual_connection:
        out = out + st.residual
    if attn.rescale_output_factor != 1.0:  # x / 1.0 == x bit-for-bit: skip the launch (always 1.0 in SD-Turbo)
        out = out / attn.rescale_output_factor
    return out


def _autocast_or(weight: torch.Tensor, x: torch.Tensor) -> torch.dtype:
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return weight.dtype


def _own_gemm(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
    """every projection shape of the SD-Turbo topology (K % 64 == 0, N % 64 == 0) runs this library's GEMMs
    (``ir_linear_fwd``: X-stationary kernels for large M at K <= 320 / K = 640, the LDS-tiled kernel for K = 1280 and
    the small-M shapes); anything else stays ``F.linear``"""
    return bool(_ops.linear_supported(x, w, bias))


def _linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], bi: bool = False) -> torch.Tensor:
    if _ops.linear_supported(x, w, bias):
        return _ops.linear(x, w, bias, batch_invariant=True) if bi else _ops.linear(x, w, bias)
    if bi:   # the vendor GEMM picks its kernel (and its summation order) from the row count
        raise NotImplementedError(f"batch-invariant mode: projection x {tuple(x.shape)} {x.dtype} @ w {tuple(w.shape)} is not covered by "
                                  "this library's GEMMs (K % 64 == 0 and N % 64 == 0, or K <= 320 / 640 with N % 32 == 0)")
    return torch.nn.functional.linear(x, w, bias)


def _module_call(bi: bool, what: str) -> None:
    """the mode's guard in front of every projection that would run as the module call itself (``nn.Linear`` -> ``F.linear``, the
    vendor GEMM, whose kernel and summation order follow the row count): it raises instead"""
    if bi:
        raise NotImplementedError(f"batch-invariant mode: {what} would run as a module call (F.linear: the vendor GEMM picks its "
                                  "kernel from the row count); only projections this library's GEMMs run are covered")


def _bi_kw(bi: bool) -> dict:
    """the keyword of the batch-invariant mode, handed to ``_ops`` only when it is on (a stand-in ``_ops`` without it keeps working)"""
    return {"batch_invariant": True} if bi else {}


LOG2E = 1.4426950408889634
FUSED_CAST = True   # own GEMM: fp32 activations (autocast) are rounded to the compute dtype while they are loaded
PRESCALE_Q = True   # own fused q/k/v GEMM: q leaves its epilogue as Q * attn.scale * log2(e) (still one rounding)


FOLD_MIN_REF_TOKENS = 8   # reference token axes shorter than this get their AdaIN applied to V (one pass) instead of folded into the kernel
FUSED_STATS = True  # own fused q/k/v GEMM: the token statistics of its V third (AdaIN) are its workgroups' tail, no pass over V


def _project_qkv(attn, st: _Prepared, want_stats: bool = False, bi: bool = False):
    """``to_q`` / ``to_k`` / ``to_v`` of the reference (attn_processors.py:222-230).  Returns
    ``(q, k, v, q_prescaled, v_stats)``; ``v_stats`` is ``None`` unless ``want_stats`` and the fused GEMM could leave
    the partial token statistics of V behind (``ops.ColumnStats``: what ``adain`` needs of V, attn_processors.py:9-10,
    :244-245, without a pass over it).

    Self-attention whose three projections are bias-free linear maps of equal shape - plain
    ``nn.Linear`` or peft LoRA wrappers in inference state (``lora_fold``) - runs them as ONE
    GEMM against a cached concatenation of the three (LoRA-folded) weights (SURVEY.md section
    8f rank 4): the fused attention kernel reads q / k / v as strided views of that single
    ``(B, L, 3C)`` result, so nothing is copied.  Same values as three separate calls for plain
    projections (each output column is the same dot product); for LoRA wrappers the adapter is
    merged exactly as peft's ``merge_and_unload`` does.  Anything else - cross attention, biased
    projections, active dropout, DoRA, training - takes the three module calls like the
    reference.

    Pre-scaled Q: when the fused GEMM is this library's own kernel (``ir_linear_fwd_scaled``), the q third of its
    output is multiplied by ``attn.scale * log2(e)`` in the fp32 accumulator, before the one rounding to 16 bit every
    projection output gets anyway.  The attention kernel is told so (``IR_FLAG_Q_PRESCALED``) and drops the
    multiply-add per score.  Shapes that go to the vendor GEMM keep the plain q."""
    src = _kv_source(attn, st)
    tq, tk, tv = attn.to_q, attn.to_k, attn.to_v
    if torch.is_grad_enabled():
        _module_call(bi, "q/k/v with autograd enabled")
        return tq(st.hidden), tk(src), tv(src), False, None
    if st.encoder is not None:
        # cross attention (the f-1 layers, attn_processors.py:224-230 with encoder_hidden_states): q from the image tokens,
        # k / v from the text states - different inputs, so no q/k/v fusion, but still this library's GEMMs (round 4: the
        # tiny-M shapes lead the vendor GEMM + its cast pass, profiles/r4_gemm_probe_small.txt) and ONE GEMM for k and v
        q = _project_single(attn, "_ir_q_cache", "_ir_q_bias_cache", tq, st.hidden, bi)
        ek, ev = _lora.effective_linear(tk), _lora.effective_linear(tv)
        if ek is not None and ev is not None and ek[0].bias is None and ev[0].bias is None and ek[0].weight.shape == ev[0].weight.shape:
            dtype = _autocast_or(ek[0].weight, src)
            w = _lora.cached_weight(attn, "_ir_kv_cache", (tk, tv), dtype)
            xs = src
            if xs.dtype != dtype and not (FUSED_CAST and _own_gemm(xs, w, None)):
                xs = xs.to(dtype)
            kv = _linear(xs, w, None, bi)
            c = w.shape[0] // 2
            return q, kv[..., :c], kv[..., c:], False, None
        _module_call(bi, "cross-attention k/v that cannot be fused")
        return q, tk(src), tv(src), False, None
    effs = [_lora.effective_linear(m) for m in (tq, tk, tv)]
    if any(e is None or e[0].bias is not None for e in effs) or \
            not (effs[0][0].weight.shape == effs[1][0].weight.shape == effs[2][0].weight.shape):
        _module_call(bi, "biased or unfoldable q/k/v projections")
        return tq(st.hidden), tk(src), tv(src), False, None
    dtype = _autocast_or(effs[0][0].weight, st.hidden)
    w = _lora.cached_weight(attn, "_ir_qkv_cache", (tq, tk, tv), dtype)
    c = w.shape[0] // 3
    x = st.hidden
    own = _own_gemm(x, w, None)      # fp32 activations go straight in: the own GEMM casts them while loading
    if x.dtype != dtype and not (own and FUSED_CAST):
        x = x.to(dtype)
    # (batch-invariant mode: the A/B tuning hook does not reach the attention, so it does not decide the q form either)
    presc = bool(PRESCALE_Q and c % 32 == 0 and own and (bi or _ops.tuning_supports_prescaled_q()))
    kw = dict(scale_cols=c, col_scale=float(attn.scale) * LOG2E) if presc else {}
    kw.update(_bi_kw(bi))
    vstats = None
    if want_stats and FUSED_STATS and own and x.dim() == 3 and c % _ops.HEAD_DIM == 0:
        # token statistics of the V third as the GEMM's tail: whole row blocks per token set (rows | L), whole heads
        rows = _ops.linear_stats_rows(x.shape[0] * x.shape[1], 3 * c, w.shape[1], False)
        if rows > 0 and x.shape[1] % rows == 0 and x.shape[1] // rows <= _ops.STATS_MAX_CHUNKS:
            qkv, vstats = _ops.linear(x, w, None, stats=(2 * c, c), **kw)
    if vstats is None:
        qkv = _ops.linear(x, w, None, **kw) if presc else _linear(x, w, None, bi)
    return qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], presc, vstats


def _project_single(attn, slot: str, bias_slot: str, module, x: torch.Tensor, bi: bool = False) -> torch.Tensor:
    """one projection module (plain ``nn.Linear`` or a foldable LoRA wrapper in inference state) as one GEMM of this library
    against its cached folded weight; the module call itself when it cannot be folded"""
    eff = _lora.effective_linear(module)
    if eff is None:
        _module_call(bi, "an unfoldable projection")
        return module(x)
    dtype = _autocast_or(eff[0].weight, x)
    w = _lora.cached_weight(attn, slot, (module,), dtype)
    bias = eff[0].bias
    if bias is not None and bias.dtype != dtype:
        bias = _lora.cached_cast(attn, bias_slot, bias, dtype)
    if x.dtype != dtype and not (FUSED_CAST and _own_gemm(x, w, bias)):
        x = x.to(dtype)
    return _linear(x, w, bias, bi)


def _project_kv_only(attn, st: _Prepared, bi: bool = False):
    """``to_k`` / ``to_v`` alone (the last K/V-capture layer under early exit): the lower two thirds of
    the cached fused weight when there is one, the two module calls otherwise."""
    src = _kv_source(attn, st)
    tk, tv = attn.to_k, attn.to_v
    if st.encoder is None and not torch.is_grad_enabled():
        effs = [_lora.effective_linear(m) for m in (attn.to_q, tk, tv)]
        if all(e is not None and e[0].bias is None for e in effs) and \
                effs[0][0].weight.shape == effs[1][0].weight.shape == effs[2][0].weight.shape:
            dtype = _autocast_or(effs[0][0].weight, st.hidden)
            w = _lora.cached_weight(attn, "_ir_qkv_cache", (attn.to_q, tk, tv), dtype)
            c = w.shape[0] // 3
            x = st.hidden
            if x.dtype != dtype and not (FUSED_CAST and _own_gemm(x, w[c:], None)):
                x = x.to(dtype)
            kv = _linear(x, w[c:], None, bi)
            return kv[..., :c], kv[..., c:]
    _module_call(bi, "k/v projections that cannot be fused")
    return tk(src), tv(src)


def _project_out(attn, tokens: torch.Tensor, bi: bool = False) -> torch.Tensor:
    """``to_out[0]`` (attn_processors.py:267): one GEMM also when the module is a LoRA wrapper in
    inference state; the module call itself in training or when it cannot be folded."""
    proj = attn.to_out[0]
    if torch.is_grad_enabled():
        _module_call(bi, "the out projection with autograd enabled")
        return proj(tokens)
    eff = _lora.effective_linear(proj)
    if eff is None:
        _module_call(bi, "an unfoldable out projection")
        return proj(tokens)
    dtype = _autocast_or(eff[0].weight, tokens)
    w = _lora.cached_weight(attn, "_ir_out_cache", (proj,), dtype)
    bias = eff[0].bias
    if bias is not None and bias.dtype != dtype:
        bias = _lora.cached_cast(attn, "_ir_out_bias_cache", bias, dtype)
    x = tokens if tokens.dtype == dtype else tokens.to(dtype)
    return _linear(x, w, bias, bi)


def _stats_cached(value: torch.Tensor, cstats, heads: int):
    """AdaIN affine from cached content statistics, reading only V_self (``ir_adain_stats_cached``)"""
    return _ops.adain_stats_cached(value, cstats[0], cstats[1], heads=heads)


def _same_16bit(q: torch.Tensor, *others: Optional[torch.Tensor]) -> List[Optional[torch.Tensor]]:
    """Under autocast the projections emit fp16/bf16; captured reference K/V have that dtype
    too.  Anything else on this path is a caller error worth hearing about."""
    res = []
    for t in others:
        if t is not None and t.dtype != q.dtype:
            raise TypeError(f"shared attention: query is {q.dtype} but a key/value tensor is {t.dtype}")
        res.append(t)
    return res


# ------------------------------------------------------------------------------------------
# K/V-capturing processor of the frozen reference UNet (attn_processors.py:22-97)
# ------------------------------------------------------------------------------------------
def _plain_setattr(self, name, value):
    """``nn.Module.__setattr__`` for modules that own no parameter, buffer or submodule (these processors: strict
    ``load_state_dict`` with an empty state, inference/test.py:47-50): plain attributes - the K/V stash, flags, events, streams -
    skip the registry walk (2 us each, ~170 per eager one-identity step: tools/gpu_host_overhead.py); anything that IS a
    parameter / module, or a name a registry already holds, takes the normal path."""
    if (type(value) in _PLAIN_VALUE_TYPES or not isinstance(value, (nn.Parameter, nn.Module))) and \
            name not in self._parameters and name not in self._buffers and name not in self._modules:
        object.__setattr__(self, name, value)
    else:
        nn.Module.__setattr__(self, name, value)


_PLAIN_VALUE_TYPES = frozenset((type(None), bool, int, float, str, list, tuple, dict, torch.Tensor))   # exact types: no registry business


class ReferenceCaptureComplete(Exception):
    """raised by the LAST K/V-capturing processor when early exit is armed (``kv_harvest``): every
    ``keys`` / ``values`` the main UNet will read is stashed, the rest of the reference UNet's forward
    only produces an output the caller throws away (inference/test.py:100)"""


class AttnProcessor(nn.Module):
    r"""Plain attention that stashes the PRE-head-split ``key`` / ``value`` projections
    ``(B*N, L, C)`` for later sharing (attn_processors.py:73-74)."""

    __setattr__ = _plain_setattr

    def __init__(self):
        super().__init__()
        self.keys, self.values = None, None
        self.is_self_attn = None
        self.stop_after_capture = None    # plain attribute (not a parameter / buffer): kv_harvest arms it with
                                          # the list of all capturing processors of the UNet
        self.record_events = False        # True: record `ready` on the current stream once K/V are stashed
        self.ready = None
        self.stream = None                # HIP stream the K/V were produced on (kv_harvest orders its zero fill after it)
        self.capture_stats = False        # True (kv_harvest.enable_ref_stats): also stash the AdaIN CONTENT statistics of
        self.v_mean, self.v_std = None, None   # every reference V, fp32 (B*N, H, 64) - constant per identity
        self.v_part = None                # ... or (round 4) the partials the q/k/v GEMM left behind (ops.ColumnStats): merged
                                          # by the shared layer's affine kernel, or into (mean, std) on demand
        self.batch_invariant = False      # ABI v10 (plain attribute; set_batch_invariant): batch-invariant GEMMs and attention
        self.capture_stats_weights = None   # kv_harvest.enable_ref_stats(..., weights=): the statistics above over WEIGHTED tokens -
                                            # a weight picture (B, N, Hpx, Wpx) or per-token weights (B, N, L), float or bool

    def reset(self):
        self.keys, self.values = None, None
        self.is_self_attn = None
        self.ready = None
        self.stream = None
        self.v_mean, self.v_std = None, None
        self.v_part = None

    def _stash_stats(self, attn, vstats=None):
        """mean and unbiased std over the tokens of every captured V, per (head, channel): the content statistics of
        ``adain`` (attn_processors.py:9-10) computed HERE, once per reference and on the capture stream, instead of in
        every shared layer of every frame.  ``vstats``: the partials the q/k/v GEMM left behind (round 4: no pass over V,
        one 64-thread-per-(set, head) merge); without them ``ir_token_stats`` reads V."""
        self.v_mean, self.v_std, self.v_part = None, None, None     # never hand a later harvest the statistics of an earlier capture
        weights = getattr(self, "capture_stats_weights", None)
        if self.capture_stats and self.values.is_cuda and weights is not None:
            # mask-aware statistics: one weighted pass over V (the GEMM's partials are unweighted); the pair travels like any other
            w = _on_grid(weights, self.values.shape[1], True, self.values.device, "adain_weights")
            if w.shape[0] * w.shape[1] != self.values.shape[0]:
                raise ValueError(f"capture_stats_weights of {tuple(w.shape)} tokens for {self.values.shape[0]} captured references")
            m, sd = _ops.token_stats_weighted(self.values.unsqueeze(1), heads=attn.heads, weights=w.reshape(-1, 1, w.shape[-1]))
            self.v_mean, self.v_std = m[:, 0], sd[:, 0]
        elif self.capture_stats and self.values.is_cuda:
            if vstats is not None:
                self.v_part = vstats       # merged where they are consumed (kv_harvest / SharedAttnProcessor): no launch here
            else:
                m, sd = _ops.token_stats(self.values.unsqueeze(1), heads=attn.heads)      # (B*N, 1, H, 64) each
                self.v_mean, self.v_std = m[:, 0], sd[:, 0]

    def _mark_ready(self):
        if self.keys.is_cuda:
            self.stream = torch.cuda.current_stream(self.keys.device)
            if self.record_events:
                self.ready = torch.cuda.Event()
                self.ready.record(self.stream)

    def forward(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None,
                ref_weights=None, ref_token_keep=None, ref_lens=None, region_labels=None, region_allow=None, adain_weights=None,
                adain_regions=None, adain_n_regions=None, adain_region_min_tokens=None):
        # ref_weights / ref_token_keep / ref_lens / region_labels / region_allow / adain_weights / adain_regions / adain_n_regions /
        # adain_region_min_tokens: accepted and ignored (no references here), like ref_valid elsewhere
        st = _prologue(attn, hidden_states, encoder_hidden_states, attention_mask, temb)
        self.is_self_attn = encoder_hidden_states is None
        group = self.stop_after_capture
        if group and all(p.keys is not None for p in group if p is not self):
            # every other capturing layer has run: this is the last one, and only its to_k / to_v are still
            # needed - no query, no attention, no out projection
            self.keys, self.values = _project_kv_only(attn, st, self.batch_invariant)
            self._stash_stats(attn)
            self._mark_ready()
            raise ReferenceCaptureComplete()
        bi = bool(self.batch_invariant)
        query, key, value, presc, vstats = _project_qkv(
            attn, st, want_stats=bool(self.capture_stats) and getattr(self, "capture_stats_weights", None) is None, bi=bi)
        self.keys, self.values = key, value  # consumed in place by the shared layers: no copies
        self._stash_stats(attn, vstats)
        self._mark_ready()
        _same_16bit(query, key, value)
        kw = {"q_prescaled": True} if presc else {}
        kw.update(_bi_kw(bi))
        bias = _mask_bias(st.mask, query.shape[0], attn.heads, key.shape[1], key.shape[1], False)
        if bias is not None:
            kw["key_bias"] = bias
        tokens = _ops.shared_attention(query, key, value, heads=attn.heads, scale=attn.scale, include_self=True, **kw)
        return _epilogue(attn, st, tokens, bi)


# ------------------------------------------------------------------------------------------
# face-embedding cross attention (attn_processors.py:100-180); off by default in the configs
# ------------------------------------------------------------------------------------------
class FaceIDAttnProcessor(nn.Module):
    def __init__(self, hidden_size, self_attn_idx=None, cross_attention_dim=None, embed_dim: int = 512):
        super().__init__()
        self.hidden_size = hidden_size
        self.cross_attention_dim = cross_attention_dim
        width = cross_attention_dim or hidden_size
        self.face_projection = nn.Linear(embed_dim, width)
        self.to_k_face_embed = nn.Linear(width, hidden_size, bias=False)
        self.to_v_face_embed = nn.Linear(width, hidden_size, bias=False)
        self.self_attn_idx = self_attn_idx
        self.keys, self.values = None, None
        self.is_self_attn = None

    def reset(self):
        self.keys, self.values = None, None
        self.is_self_attn = None

    def forward(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None,
                ref_keys=None, ref_values=None, ref_events=None, ref_stats=None, ref_valid=None, ref_weights=None, ref_token_keep=None,
                ref_lens=None, region_labels=None, region_allow=None, adain_weights=None,
                adain_regions=None, adain_n_regions=None, adain_region_min_tokens=None):
        # ref_* / region_* / adain_weights / adain_regions (with its two settings) accepted and ignored, like the reference: the host forwards ONE cross_attention_kwargs dict to every processor
        # (unet.py / diffusers), so whatever the harvest hands SharedAttnProcessor (ref_valid included) arrives here too
        st = _prologue(attn, hidden_states, encoder_hidden_states, attention_mask, temb)
        self.is_self_attn = encoder_hidden_states is None
        query = attn.to_q(st.hidden)
        src = self.face_projection(_kv_source(attn, st))
        key, value = self.to_k_face_embed(src), self.to_v_face_embed(src)
        _same_16bit(query, key, value)
        bias = _mask_bias(st.mask, query.shape[0], attn.heads, key.shape[1], key.shape[1], False)
        kw = {"key_bias": bias} if bias is not None else {}
        tokens = _ops.shared_attention(query, key, value, heads=attn.heads, scale=attn.scale, include_self=True, **kw)
        return _epilogue(attn, st, tokens)


# ------------------------------------------------------------------------------------------
# the read-outs of a shared layer: one declaration each; refusals, validation, want_lse and the launches follow the table
# ------------------------------------------------------------------------------------------
class _Readout(NamedTuple):
    switch: str                     # the attribute that switches it on: anything but None, on shared layers (see ``flag``)
    entry: str                      # the C entry point, as the refusals name it
    op: str                         # the ``_ops`` function: op(query, key, ref_k, lse, *args, heads=, scale=, include_self=, ...)
    result: str                     # the attribute that receives what it returns
    listed: int                     # its place among the names of the region refusal
    args: Tuple[str, ...] = ()      # attributes handed on after ``lse``, in order
    sentinel: Optional[str] = None  # the string the LAST of ``args`` may be instead of a tensor (handed on as None: every token)
    takes: str = "an integer tensor"    # ... and what it is otherwise, for the message
    reduce: Optional[str] = None    # its ``*_reduce`` attribute (default "head_mean"); the switch itself: validated here
    extra: Tuple[Tuple[str, str, object], ...] = ()    # further (keyword, attribute, default)
    flag: bool = False              # the switch is a bool instead, honoured on every layer (the dump)
    paired: bool = False            # shares one message per rule with the other paired rows


# in launch order: a captured step contains the launches in this order
_READOUTS = (
    _Readout("attention_rows_index", "ir_attn_rows", "attn_rows", "attention_rows", 1, args=("attention_rows_index",),
             reduce="attention_rows_reduce", paired=True),
    _Readout("attention_match_index", "ir_attn_match", "attn_match", "attention_match", 2, args=("attention_match_index",), sentinel="all",
             reduce="attention_match_reduce"),
    _Readout("attention_transfer_payload", "ir_attn_transfer", "attn_transfer", "attention_transfer", 4,
             args=("attention_transfer_payload", "attention_transfer_index"), sentinel="all", reduce="attention_transfer_reduce"),
    _Readout("attention_received_weights", "ir_attn_received", "attn_received", "attention_received", 5, args=("attention_received_weights",),
             sentinel="ones", takes="an fp32 tensor", reduce="attention_received_reduce"),
    _Readout("attention_topk_index", "ir_attn_topk", "attn_topk", "attention_topk", 3, args=("attention_topk_index",), sentinel="all",
             reduce="attention_topk_reduce", extra=(("k", "attention_topk_k", 4),)),
    _Readout("attention_key_match_reduce", "ir_attn_key_match", "attn_key_match", "attention_key_match", 6, reduce="attention_key_match_reduce"),
    # (B, H, L, Lkv), columns [self?] ++ ref0 ++ ... ++ refN-1, in the compute dtype: launched last, refused and listed first
    _Readout("save_self_attentions", "ir_attn_probs", "attn_probs", "attention_probs", 0, flag=True, paired=True),
)
_REDUCES = ("none", "head_mean")
LN2 = 0.6931471805599453    # a pre-scaled query carries scale * log2(e): its scores are exponents, ln 2 turns them into the logits of the LSE


_SWITCHES = tuple((r.switch, r.flag, r) for r in _READOUTS)     # (every call of every layer walks the switches: no field lookups)


def _readouts_on(proc, shared: bool):
    """the rows of the table that this call of ``proc`` launches, in launch order"""
    if shared:
        return [r for n, flag, r in _SWITCHES if (getattr(proc, n, None) if flag else getattr(proc, n, None) is not None)]
    return [r for n, flag, r in _SWITCHES if flag and getattr(proc, n, None)]


def _rule_text(row: _Readout, text: str) -> str:
    """``text`` about ``row`` - or about the pair ``save_self_attentions / attention_rows_index``, which shares one"""
    rows = sorted((r for r in _READOUTS if r.paired), key=lambda r: r.listed) if row.paired else [row]
    text = text.format(names=" / ".join(r.switch for r in rows), entries=" and ".join(r.entry for r in rows))
    return text.replace(" does not ", " do not ") if row.paired else text      # (two kernels: the plural)


def _refuse(proc, on, *, biased: bool, counts, cstats, ref_v, ref_valid, region_labels, region_allow, adain_weights, adain_regions,
            adain_n_regions) -> None:
    """every refusal that the kwargs and the attributes decide, before anything is launched.  ``on``: the read-outs of this call;
    ``biased``: a mask, ``ref_weights`` or ``ref_token_keep`` will make a key bias; ``counts`` / ``cstats`` / ``ref_v``: this layer's
    entries of ``ref_lens`` / ``ref_stats`` / ``ref_values`` (``None`` on a layer that shares nothing, like the four kwargs)"""
    first = next((r for r in on if r.paired), on[0]) if on else None     # the read-out a rule names: the pair's message leads
    if region_labels is not None:
        if region_allow is None:
            raise ValueError("region_labels needs region_allow: the (C, C) bool matrix or the (C,) bitmasks of ops.region_masks")
        if biased:
            raise NotImplementedError("region_labels together with an attention mask, ref_weights or ref_token_keep: the kernel carries either "
                                      "the key bias or the region test; regions with a key bias are a follow-up")
        if counts is not None:
            raise NotImplementedError("region_labels together with ref_lens: key_region indexes the packed uniform key axis; regions with "
                                      "per-reference counts are a follow-up")
        if on:
            raise NotImplementedError(f"region_labels together with {', '.join(r.switch for r in sorted(on, key=lambda r: r.listed))}: "
                                      "the read-out kernels do not take regions yet (their exp(s - lse) would count the pairs the forward "
                                      "left out; follow-up); save_attention_mass honours the regions")
    if adain_regions is not None:
        if adain_n_regions is None:
            raise ValueError("adain_regions needs adain_n_regions (1 ... 32): inferring it from the labels would need a device sync")
        if adain_weights is not None:
            raise NotImplementedError("adain_regions together with adain_weights: regional statistics over weighted tokens are a follow-up")
        if counts is not None:
            raise NotImplementedError("adain_regions together with ref_lens: the labels index the uncompacted token axis; regions "
                                      "over compacted references are a follow-up")
        if isinstance(ref_v, _RefKVTable):
            raise NotImplementedError("adain_regions with RefKVTable references: the regional statistics and the renormalised V need "
                                      "dense references; cached per-identity regional statistics are the follow-up")
    if counts is not None:
        if ref_valid is not None:
            raise ValueError("ref_lens with ref_valid: a count of 0 says the reference is absent, ref_valid says it is zero-filled "
                             "(its tokens keep exp(0)) - pass one of the two")
        if biased:
            raise NotImplementedError("ref_lens together with an attention mask, ref_weights or ref_token_keep: the key bias indexes the "
                                      "packed uniform key axis; counts with a bias are a follow-up (compact the kept tokens instead)")
        if first is not None:
            raise NotImplementedError(_rule_text(first, "ref_lens together with {names}: {entries} would walk the tails behind the counts (follow-up)")
                                      + ("; save_attention_mass honours the counts" if first.paired else ""))
        if proc.use_adain and cstats is None:
            raise ValueError("ref_lens with use_adain needs ref_stats: the AdaIN content statistics are those of the full reference, "
                             "taken before compaction - computing them here would read the packed rows and whatever lies behind them")
    for row in on:
        if row.sentinel is not None:
            v = getattr(proc, row.args[-1], None)
            if isinstance(v, str) and v != row.sentinel:
                raise ValueError(f"{row.args[-1]} must be None, \"{row.sentinel}\" or {row.takes}, got {v!r}")
        if row.reduce == row.switch and getattr(proc, row.switch) not in _REDUCES:
            raise ValueError(f"{row.switch} must be None, \"none\" or \"head_mean\", got {getattr(proc, row.switch)!r}")
    if biased and first is not None:
        raise NotImplementedError(_rule_text(first, "{names} together with an attention mask, ref_weights or ref_token_keep: "
                                                       "{entries} does not take the key bias yet (follow-up)")
                                  + ("; save_attention_mass honours it" if first.paired else ""))


def _read_out(proc, on, query, key, ref_k, lse, **kw) -> None:
    """launches the read-outs ``on`` from the LSE of the attention call, in the table's order, and leaves each result on ``proc``"""
    for row in on:
        args = [getattr(proc, n, None) for n in row.args]
        if row.sentinel is not None and isinstance(args[-1], str):
            args[-1] = None
        rkw = dict(kw)
        if row.reduce is not None:
            rkw["reduce"] = getattr(proc, row.reduce, "head_mean")
        for name, attribute, default in row.extra:
            rkw[name] = getattr(proc, attribute, default)
        setattr(proc, row.result, getattr(_ops, row.op)(query, key, ref_k, lse, *args, **rkw))


def _adain_step(attn, value, ref_v, ref_valid, cstats, vstats, adain_weights, adain_regions, adain_n_regions, adain_region_min_tokens):
    """AdaIN of a shared layer with ``use_adain`` -> ``(affine, ref_v, ref_valid)``: the affine ``(a, b)`` that the attention folds in,
    or ``None`` beside a renormalised ``ref_v`` where the affine was applied to V here.

    style = this image's own post-projection V; content = each reference V.  With the content statistics handed over
    (``cstats``, from ``ref_stats``: computed once per identity by the K/V-capture layer, kv_harvest with_stats) only V_self is
    read here - 1/(N+1) of the bytes, the same (a, b) bit for bit.  Round 4: the style statistics arrive as the partials this
    layer's own q/k/v GEMM left behind (``vstats``): with them and the content statistics nothing of V is read here at all - one
    small launch."""
    affine = None
    geometry = (value.shape[0], value.shape[1], ref_v.shape[1], ref_v.shape[2])
    if adain_regions is not None:
        # per-region AdaIN: one affine per (reference, region) cannot ride the fold (it applies a * sum(p v) + b * sum(p)
        # once per segment), so the renormalised V is formed here - the reference's own order of operations - and
        # the attention runs without an affine
        R = int(adain_n_regions)
        q_lab, r_lab = _adain_region_labels(adain_regions, *geometry, value.device)
        v1 = value.unsqueeze(1)
        style_g = _ops.token_stats(v1, heads=attn.heads)
        style_r = _ops.token_stats_regions(v1, q_lab.unsqueeze(1), heads=attn.heads, n_regions=R, return_count=True)
        content_g = _ops.token_stats(ref_v, heads=attn.heads)
        content_r = _ops.token_stats_regions(ref_v, r_lab, heads=attn.heads, n_regions=R, return_count=True)
        table = _ops.adain_affine_regions(style_r, content_r, style_g, content_g,
                                          min_tokens=FOLD_MIN_REF_TOKENS if adain_region_min_tokens is None else adain_region_min_tokens)
        # a zero-filled reference's V is the style mean now, not zero: its tiles are walked
        return None, _ops.adain_apply_regions(ref_v, r_lab, table[0], table[1], heads=attn.heads), None
    if adain_weights is not None:
        # mask-aware AdaIN: the style statistics over this layer's weighted tokens; the content statistics as the
        # caller finished them (``ref_stats``), else over the dense references' weighted tokens
        self_w, ref_w = _adain_weight_pair(adain_weights, *geometry, value.device)
        if hasattr(cstats, "finished"):
            content = cstats.finished()
        elif cstats is not None:
            content = cstats
        elif isinstance(ref_v, _RefKVTable):
            raise ValueError("use_adain with RefKVTable references needs ref_stats: cache the identities with their AdaIN content "
                             "statistics (get_conditioning_keys_values(..., with_stats=True[, stats_weights=...])) and pass the "
                             "stats of ReferenceKVCache.assemble_tables")
        else:
            content = _ops.token_stats_weighted(ref_v, heads=attn.heads, weights=ref_w)
        style = _ops.token_stats_weighted(value.unsqueeze(1), heads=attn.heads,
                                          weights=None if self_w is None else self_w.unsqueeze(1))
        affine = _ops.adain_affine(style, content)
    elif hasattr(cstats, "finished"):
        if vstats is not None:    # both sides as partials: ONE launch merges them into the affine
            affine = _ops.adain_affine_from_partials(vstats, *geometry, content=cstats.part, valid=cstats.valid)
        else:
            affine = _stats_cached(value, cstats.finished(), attn.heads)
    elif cstats is not None and vstats is not None:
        affine = _ops.adain_affine_from_partials(vstats, *geometry, content_mean=cstats[0], content_std=cstats[1])
    elif cstats is not None:
        affine = _stats_cached(value, cstats, attn.heads)
    elif isinstance(ref_v, _RefKVTable):
        # the content statistics would need a pass over every reference V, and ir_adain_stats reads a dense tensor:
        # a table is never densified behind the caller's back
        raise ValueError("use_adain with RefKVTable references needs ref_stats: cache the identities with their AdaIN content "
                         "statistics (get_conditioning_keys_values(..., with_stats=True)) and pass the stats of "
                         "ReferenceKVCache.assemble_tables")
    else:
        affine = _ops.adain_stats(value, ref_v, heads=attn.heads)
    if ref_v.shape[2] >= FOLD_MIN_REF_TOKENS:
        return affine, ref_v, ref_valid
    if isinstance(ref_v, _RefKVTable):
        raise ValueError(f"RefKVTable references of fewer than {FOLD_MIN_REF_TOKENS} tokens with use_adain: this branch forms the "
                         "renormalised V as a dense tensor; pass dense ref_values (the model's own axes never come here)")
    # a handful of reference tokens: a channel whose few values lie ulps apart gets a ratio in the thousands, and the
    # fold's a * sum(p~ v) + b * sum(p) would amplify the 16-bit rounding of P by a * |mean|.  Here the
    # renormalised V is formed once (ir_adain_apply, fp32 arithmetic, one rounding - what the reference's adain()
    # does, attn_processors.py:7-18) and the attention runs without an affine.  Never taken by the model's own axes (>= 256).
    # A zero-filled reference's V is the style mean now, not zero: its tiles are walked
    return None, _ops.adain_apply(ref_v, affine[0], affine[1], heads=attn.heads), None


# ------------------------------------------------------------------------------------------
# the hot path: shared-image attention (attn_processors.py:183-279)
# ------------------------------------------------------------------------------------------
class SharedAttnProcessor(nn.Module):
    r"""Extended self-attention over ``[self K/V (iff train_input)] ++ N x reference K/V``.

    ``ref_keys[self_attn_idx]`` / ``ref_values[...]`` are the ``(B, N, L, C)`` tensors produced
    by ``get_conditioning_keys_values`` (pix2pix_turbo.py:265-266) - or ``ops.RefKVTable`` pointer tables over per-identity cache
    entries (``ReferenceKVCache.assemble_tables``: no ``(B, N, L, C)`` copy; with ``use_adain`` they need ``ref_stats``); they are read in place by the
    kernel (segment walk) - N is taken from the tensor, zero-filled references keep their
    ``exp(0)`` weight, and with ``use_adain`` every reference V is renormalised to the
    statistics of this image's own V inside the kernel's V staging.
    """

    __setattr__ = _plain_setattr

    def __init__(self, self_attn_idx: int = None, save_self_attentions: bool = False,
                 use_adain: bool = False, train_input: bool = True):
        super().__init__()
        self.self_attn_idx = self_attn_idx
        self.save_self_attentions = save_self_attentions
        self.use_adain = use_adain
        self.train_input = train_input
        # opt-in (round 5; a plain attribute like ``AttnProcessor.record_events``, the constructor stays the reference's): when set,
        # every call also leaves ``attention_mass`` - fp32 (B, H, L, [self?] + N), the attention mass per K/V segment - which is what
        # gradio_demo.py:119-127 reduces ``attention_probs`` to (``probs[..., attn_size*idx : attn_size*(idx+1)].sum(-1)``), without
        # the (B, H, L, Lkv) tensor and without a second pass (``ir_shared_attn_args.seg_mass``, ABI v9).  Independent of ``save_self_attentions``, whose meaning is unchanged.
        # COLUMN ORDER vs the reference's demo: gradio_demo.py slices blocks ``attn_size*idx`` for idx 0..3 starting at column 0.  With
        # ``train_input`` the columns are [self, ref0, ref1, ...], so the demo's block 0 is the SELF segment and its last reference is
        # never read.  Reference-parity ranking therefore uses ``attention_mass[..., 0:4]`` (meaningful only when Ls == Lr, which the
        # model guarantees); ``attention_mass[..., int(train_input):]`` is the per-REFERENCE form (what the demo presumably meant).
        self.save_attention_mass = False
        self.attention_mass = None
        # ABI v10 (plain attribute; set_batch_invariant): every GEMM and attention of this processor runs the library's batch-invariant
        # plans - an identity's output, attention_mass and attention_probs do not depend on the rest of its batch
        self.batch_invariant = False
        # opt-in (plain attributes like ``save_attention_mass``): ``attention_rows_index`` - an integer tensor ``(R,)`` or ``(B, R)`` of
        # query tokens, e.g. ``attn_maps.landmark_rows(...)`` - makes every call of a shared layer leave ``attention_rows``: the
        # probability rows of those tokens (``ir_attn_rows``), reduced as ``attention_rows_reduce`` says - "none": ``attention_probs[:, :, idx]``
        # (B, H, R, Lkv); "head_mean": fp32 (B, R, Lkv), ``attn.mean(dim=1)[b][idx]``; "map": fp32 (B, Lkv), their sum - what
        # vis_utils.py:88-110 reads out of ``attention_probs``, without the (B, H, L, Lkv) tensor.  Independent of
        # ``save_self_attentions`` (with both set, the one LSE of the attention call serves both).  ``None``: off, nothing changes.
        self.attention_rows_index = None
        self.attention_rows_reduce = "head_mean"
        self.attention_rows = None
        # opt-in (plain attributes like ``attention_rows_index``): ``attention_match_index`` - ``"all"`` (every query token) or an integer
        # tensor ``(R,)`` / ``(B, R)`` - makes every call of a shared layer leave ``attention_match = (index, prob)``: per K/V segment the
        # largest probability of each chosen token and the key, counted inside its segment, that attains it (``ir_attn_match``) -
        # ``attention_probs[..., segment].max(-1)`` / ``.argmax(-1)`` without the (B, H, L, Lkv) tensor.  ``attention_match_reduce``:
        # "head_mean" - int32 / fp32 (B, R, S), of the head mean; "none" - (B, H, R, S), per head.  ``attn_maps.match_coordinates`` /
        # ``match_field`` turn the indices into grid positions.  Uses the LSE of the same attention call.  ``None``: off, nothing changes.
        self.attention_match_index = None
        self.attention_match_reduce = "head_mean"
        self.attention_match = None
        # opt-in (plain attributes like ``attention_match_index``): ``attention_transfer_payload`` - an fp32 device tensor ``(Lkv, C)``,
        # ``(1, Lkv, C)`` or ``(B, Lkv, C)`` over the key axis, C <= 8 (``attn_maps.coordinate_payload`` / ``image_payload``) - makes every
        # call of a shared layer leave ``attention_transfer = (sums, mass)``: per K/V segment the attention-weighted sum of the payload
        # and the segment's mass (``ir_attn_transfer``) - ``einsum('bhij,bjc->bhic')`` over a segment's columns of ``attention_probs``
        # without the (B, H, L, Lkv) tensor.  ``attention_transfer_index``: ``None`` / ``"all"`` (every query token) or an integer tensor
        # ``(R,)`` / ``(B, R)``.  ``attention_transfer_reduce``: "head_mean" - fp32 (B, R, S, C) / (B, R, S); "none" - (B, H, R, S, C) /
        # (B, H, R, S).  ``attn_maps.soft_match_field`` turns the sums of a coordinate payload into expected positions.  Uses the LSE of
        # the same attention call.  ``None`` payload: off, nothing changes.
        self.attention_transfer_payload = None
        self.attention_transfer_index = None
        self.attention_transfer_reduce = "head_mean"
        self.attention_transfer = None
        # opt-in (plain attributes like ``attention_transfer_payload``): ``attention_received_weights`` - ``"ones"`` or an fp32 device
        # tensor over the QUERY axis, ``(L, C)``, ``(1, L, C)`` or ``(B, L, C)``, C <= 8 (``(L,)`` / ``(B, L)``: one channel) - makes every
        # call of a shared layer leave ``attention_received``: per key of the packed key axis the sum over ALL query tokens of the
        # attention times the weights (``ir_attn_received``) - ``einsum('bhij,bic->bhjc', attention_probs, w)``, with "ones"
        # ``attention_probs.sum(-2)``, without the (B, H, L, Lkv) tensor.  ``attention_received_reduce``: "head_mean" - fp32
        # (B, Lkv, C); "none" - (B, H, Lkv, C).  ``attn_maps.received_maps`` cuts it into pictures, ``keep_from_received`` into a
        # ``keep`` mask for ``ops.compact_refs``.  Uses the LSE of the same attention call.  ``None``: off, nothing changes.
        self.attention_received_weights = None
        self.attention_received_reduce = "head_mean"
        self.attention_received = None
        # opt-in (plain attributes like ``attention_match_index``): ``attention_topk_index`` - ``"all"`` (every query token) or an integer
        # tensor ``(R,)`` / ``(B, R)`` - makes every call of a shared layer leave ``attention_topk = (index, prob)``: per K/V segment the
        # ``attention_topk_k`` (1 ... 8, default 4) largest probabilities of each chosen token and the keys, counted inside their segment,
        # that attain them, under (probability descending, key ascending) (``ir_attn_topk``) - ``torch.topk`` over a segment's columns of
        # ``attention_probs`` without the (B, H, L, Lkv) tensor; rank 0 is ``attention_match``.  ``attention_topk_reduce``: "head_mean" -
        # int32 / fp32 (B, R, S, k), of the head mean; "none" - (B, H, R, S, k), per head.  ``attn_maps.topk_coordinates`` /
        # ``match_ambiguity`` / ``topk_coverage`` / ``keep_from_topk`` read the result.  Uses the LSE of the same attention call.
        # ``None``: off, nothing changes.
        self.attention_topk_index = None
        self.attention_topk_k = 4
        self.attention_topk_reduce = "head_mean"
        self.attention_topk = None
        # opt-in (plain attributes like ``attention_received_weights``): ``attention_key_match_reduce`` - "head_mean" or "none" - makes
        # every call of a shared layer leave ``attention_key_match = (index, prob)``: per key of the packed key axis the largest
        # probability over ALL query tokens and the LOWEST query token that attains it (``ir_attn_key_match``) -
        # ``attention_probs.max(-2)`` / ``.argmax(-2)`` without the (B, H, L, Lkv) tensor.  "head_mean" - int32 / fp32 (B, Lkv), of the
        # head mean; "none" - (B, H, Lkv), per head.  With ``attention_match_index = "all"`` and the same reduce,
        # ``attn_maps.mutual_matches`` / ``mutual_match_field`` keep the pairs that pass the mutual check; ``keep_from_key_match`` turns
        # ``prob`` into a ``keep`` mask for ``ops.compact_refs``.  Uses the LSE of the same attention call.  ``None``: off, nothing changes.
        self.attention_key_match_reduce = None
        self.attention_key_match = None

    def forward(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None,
                ref_keys=None, ref_values=None, ref_events=None, ref_stats=None, ref_valid=None, ref_weights=None, ref_token_keep=None,
                ref_lens=None, region_labels=None, region_allow=None, adain_weights=None,
                adain_regions=None, adain_n_regions=None, adain_region_min_tokens=None):
        """``attention_mask``: additive, ``(B, Lkv)``, ``(B, 1, Lkv)`` or ``(B * H, 1, Lkv)`` over this layer's key axis (with references: the
        extended one) - the fused kernel's key bias.  ``ref_weights`` ``(B, N)`` >= 0 and ``ref_token_keep`` (bool ``(B, N, len_ref)`` or
        ``(B, N, S, S)``), shared layers only (ignored elsewhere, as ``ref_valid`` is): ``ops.key_bias`` turns them into the bias -
        ``log w`` on a reference's keys, 0 / dropped tokens MASKED (no attention at all, unlike a zero-filled reference).  AdaIN
        statistics stay those of every reference token unless ``adain_weights`` (below) says otherwise.  ``save_attention_mass`` reads the effect back; ``save_self_attentions`` /
        ``attention_rows_index`` (and every other read-out) with a bias raise (the read-out kernels do not take the bias yet).

        ``ref_valid`` (optional, round 5): int32 ``(B,)`` device tensor from the harvest (``kv_harvest`` ``with_valid``) when
        it zero-filled references ``n >= valid[b]`` (pix2pix_turbo.py:269-273): the kernel then closes those all-zero segments
        analytically instead of walking them (ABI v8 ``valid_refs``).  Same output; the tokens keep their exp(0) weight.

        ``ref_lens`` (optional), shared layers only (ignored elsewhere, as ``ref_valid`` is): a list with one int32 ``(B, N)`` device
        tensor per shared layer (or ``None``) - the number of keys every reference HAS (``ops.compact_refs``,
        ``ReferenceKVCache.assemble_tables``); the reference tensors' token axis is then only their capacity, and the kernel walks the
        existing keys alone (``ir_shared_attn_ragged_args``).  Raises with ``ref_valid`` (absent is not zero-filled), with a mask /
        ``ref_weights`` / ``ref_token_keep`` (counts with a key bias are a follow-up; ``ref_token_keep`` alone keeps running the bias
        path), with ``save_self_attentions`` and ``attention_rows_index`` (the read-out kernels would read on behind the counts);
        ``save_attention_mass`` works.  With ``use_adain`` it needs ``ref_stats``: by default the content statistics of the FULL
        reference, taken before compaction - the rule of the bias path, so a compacted call and a masked call agree - or, with
        ``adain_weights``, kept-token statistics (``ops.token_stats_weighted(packed_v, heads=H, lens=lens)``).

        ``region_labels = (query_labels, ref_labels)`` with ``region_allow`` (optional), shared layers only (ignored elsewhere, as
        ``ref_valid`` is): a per-QUERY restriction by class labels - "eye tokens draw from eye tokens of the references".  The labels
        are integer label pictures (``(B, Hpx, Wpx)`` of this image, ``(B, N, Hpx, Wpx)`` of its references: a face parsing map) or
        per-token labels of a square grid (``(B, L)`` / ``(B, N, L)``); every layer samples them at its own token centres
        (``attn_maps.token_labels``).  ``region_allow`` is the rule of ``ops.region_masks``: a ``(C, C)`` bool matrix (row = query class,
        column = key class) or ``(C,)`` bitmasks, at most 31 classes.  With ``train_input`` the self keys carry the query labels and
        every token sees its own picture whatever the rule (``self_free``).  The pair ``(q_allow, key_region)`` is built
        once per key-axis geometry and cached by tensor identity and version.  AdaIN is unchanged (see ``adain_weights``); ``save_attention_mass`` honours the
        regions.  Raises, before anything is launched, with an attention mask, ``ref_weights``, ``ref_token_keep`` or ``ref_lens``
        (regions with a key bias or with counts are a follow-up) and with ``save_self_attentions`` or any read-out attribute (the
        read-out kernels do not take regions yet); with ``ref_valid`` a dense call walks the zero-filled references, a table call raises.

        ``adain_weights = (self_weights, ref_weights)`` (optional; either may be ``None``), shared layers with ``use_adain`` only
        (accepted and ignored elsewhere, as ``ref_valid`` is): mask-aware AdaIN - the statistics behind the affine are taken over
        weighted tokens (``ops.token_stats_weighted``: weight 0 drops a token, 0/1 weights give the statistics of the kept tokens
        alone).  Each element is a weight picture (``(B, Hpx, Wpx)`` of this image, ``(B, N, Hpx, Wpx)`` of its references) or
        per-token weights of a square grid (``(B, L)`` / ``(B, N, L)``), float or bool; every layer samples them at its own token
        centres (``attn_maps.token_weights``), once per geometry, cached by tensor identity and version.  The style statistics are
        one weighted pass over this layer's V (the GEMM's statistics tail is not used: its partials are unweighted).  The content
        statistics are ``ref_stats`` of this layer when given - finished by the caller with the weights they wanted, e.g.
        ``ops.token_stats_weighted(packed_v, lens=lens)`` after a compaction; the pair's reference weights are then not consulted -
        otherwise one weighted pass over the dense reference V; a ``RefKVTable`` without ``ref_stats`` raises as without the
        kwarg, and so does ``ref_lens`` without ``ref_stats``.  The affine comes from ``ops.adain_affine`` and enters the
        attention as any other: masks, ``ref_weights``, ``ref_token_keep``, regions and the batch-invariant mode work with it.

        ``adain_regions = (query_labels, ref_labels)`` with ``adain_n_regions`` (required: inferring it would need a sync) and the
        optional ``adain_region_min_tokens`` (default 8), shared layers with ``use_adain`` only (accepted and ignored elsewhere):
        per-REGION AdaIN - eye tokens of a reference are renormalised with eye statistics, skin with skin.  The labels are
        integer label pictures (``(B, Hpx, Wpx)`` / ``(B, N, Hpx, Wpx)``: a face parsing map, the one ``region_labels`` takes) or
        per-token labels of a square grid (``(B, L)`` / ``(B, N, L)``), sampled by every layer at its own token centres
        (``attn_maps.token_labels``), once per geometry, cached by tensor identity and version.  A label outside
        ``[0, adain_n_regions)`` is "no region": such a token takes the whole-face affine.  The fold cannot carry an affine per key,
        so this is the apply-to-V branch: the GEMM's statistics tail is off; style and content statistics are
        ``ops.token_stats`` + ``ops.token_stats_regions`` over this layer's V and over the dense reference V; the table comes from
        ``ops.adain_affine_regions`` (a region with fewer than ``adain_region_min_tokens`` tokens on either side falls back to the
        whole-face affine); ``ops.adain_apply_regions`` forms the renormalised V once and the attention runs on it WITHOUT an affine
        and without ``ref_valid`` (a zero-filled reference's V is the style mean now: its tiles are walked).  Masks, ``ref_weights``,
        ``ref_token_keep``, ``region_labels``, ``save_attention_mass``, the read-outs and the batch-invariant mode see an ordinary
        call.  ``ref_stats`` is not consulted.  Raises, before anything is launched: without ``adain_n_regions`` (ValueError); with
        ``adain_weights`` (regional statistics over weighted tokens are a follow-up), with ``ref_lens`` (the labels index the
        uncompacted token axis; a follow-up) and with ``RefKVTable`` references (cached per-identity regional statistics are the
        follow-up) - NotImplementedError.

        Every refusal above that the kwargs and the processor's attributes decide comes before anything is launched (``_refuse``):
        the q/k/v projection of a refused call does not run.  The read-outs and what each needs are the rows of ``_READOUTS``."""
        st = _prologue(attn, hidden_states, encoder_hidden_states, attention_mask, temb)
        idx = self.self_attn_idx
        shared = idx is not None and ref_keys is not None and ref_values is not None
        bi = bool(getattr(self, "batch_invariant", False))
        use_adain = bool(shared and self.use_adain)
        ref_k = ref_v = cstats = counts = None     # this layer's entries of ref_keys / ref_values / ref_stats / ref_lens
        if shared:
            ref_k, ref_v = ref_keys[idx], ref_values[idx]
            cstats = ref_stats[idx] if ref_stats is not None else None
            counts = ref_lens[idx] if ref_lens is not None else None
        else:       # a layer that shares nothing ignores what belongs to the references
            ref_valid = ref_weights = ref_token_keep = region_labels = None
        if not use_adain:
            adain_weights = adain_regions = None
        on = _readouts_on(self, shared)
        if on or counts is not None or region_labels is not None or adain_regions is not None:      # (no rule is about anything else)
            _refuse(self, on, biased=st.mask is not None or ref_weights is not None or ref_token_keep is not None, counts=counts,
                    cstats=cstats, ref_v=ref_v, ref_valid=ref_valid, region_labels=region_labels, region_allow=region_allow,
                    adain_weights=adain_weights, adain_regions=adain_regions, adain_n_regions=adain_n_regions)

        # the GEMM's statistics tail (style partials of this layer's own V) only pays when the content statistics arrive
        # precomputed (``ref_stats``): without them ir_adain_stats reads every V anyway and would throw the partials away.
        # Mask-aware and per-region AdaIN take statistics passes of their own
        query, key, value, presc, vstats = _project_qkv(
            attn, st, want_stats=use_adain and cstats is not None and adain_weights is None and adain_regions is None, bi=bi)

        include_self = True
        if shared:
            include_self = bool(self.train_input)
            if ref_events is not None and ref_events[idx] is not None:
                # the reference UNet runs on another HIP stream (kv_harvest with_events): this layer needs
                # capture layer `self_attn_idx` and nothing later
                cur = torch.cuda.current_stream(ref_k.device)
                cur.wait_event(ref_events[idx])
                ref_k.record_stream(cur)
                ref_v.record_stream(cur)
                if hasattr(cstats, "finished"):
                    cstats.record_stream(cur)
                elif cstats is not None:
                    cstats[0].record_stream(cur)
                    cstats[1].record_stream(cur)
            elif hasattr(cstats, "sync_to_current"):
                cstats.sync_to_current()      # no event handed over: order this stream behind the partials' producer (no-op on one stream)
        _same_16bit(query, key, value, ref_k, ref_v)

        affine = None
        if use_adain:
            affine, ref_v, ref_valid = _adain_step(attn, value, ref_v, ref_valid, cstats, vstats, adain_weights, adain_regions,
                                                   adain_n_regions, adain_region_min_tokens)

        kw = {"q_prescaled": True} if presc else {}
        kw.update(_bi_kw(bi))
        if ref_valid is not None:
            kw["valid_refs"] = ref_valid
        if counts is not None:
            kw["ref_lens"] = counts
        len_self = key.shape[1]
        lkv = (len_self if include_self else 0) + (ref_k.shape[1] * ref_k.shape[2] if shared else 0)
        bias = _mask_bias(st.mask, query.shape[0], attn.heads, lkv, len_self, shared)
        if shared:
            row = _ref_bias_row(ref_weights, ref_token_keep, query.shape[0], len_self, ref_k.shape[1], ref_k.shape[2], include_self, query.device)
            if row is not None:
                bias = row if bias is None else (bias + (row if bias.dim() == 2 else row.unsqueeze(1)))
        if bias is not None:
            kw["key_bias"] = bias
        if region_labels is not None:
            kw["q_allow"], kw["key_region"] = _region_pair(region_labels, region_allow, query.shape[0],
                                                           query.shape[1], len_self, ref_k.shape[1], ref_k.shape[2], include_self, query.device)

        # the masses are a by-product of the attention launch itself (ABI v9 ``seg_mass``: the kernels hold the row sums at every
        # segment boundary): no second pass over Q and K.  Every read-out works from the one LSE of this launch
        want_lse = bool(on)
        want_mass = bool(getattr(self, "save_attention_mass", False))
        res = _ops.shared_attention(query, key, value, ref_k, ref_v, heads=attn.heads, scale=attn.scale,
                                    include_self=include_self, adain=affine, return_lse=want_lse, return_mass=want_mass, **kw)
        if want_mass:
            self.attention_mass = res[-1]
            res = res[:-1] if want_lse else res[0]
        if want_lse:
            tokens, lse = res
        else:
            tokens = res

        if on:
            _read_out(self, on, query, key, ref_k, lse, heads=attn.heads, scale=LN2 if presc else attn.scale, include_self=include_self,
                      **_bi_kw(bi))
        return _epilogue(attn, st, tokens, bi)


# ------------------------------------------------------------------------------------------
# registration: the plugin boundary (attn_processors.py:282-331)
# ------------------------------------------------------------------------------------------
def _hidden_size_for(name: str, block_out_channels) -> Optional[int]:
    if name.startswith("mid_block"):
        return block_out_channels[-1]
    if name.startswith("up_blocks"):
        return list(reversed(block_out_channels))[int(name[len("up_blocks.")])]
    if name.startswith("down_blocks"):
        return block_out_channels[int(name[len("down_blocks.")])]
    return None


def register_attention_processor(unet, cfg, save_self_attentions: bool = False):
    """Install a :class:`SharedAttnProcessor` on every attention of the main UNet.

    Walks ``unet.attn_processors`` in registration order; the ``up_blocks.*attn1`` layers get
    ``self_attn_idx`` 0..8 (``up_blocks.1.attentions.{0,1,2}``, then ``.2``, then ``.3``); all
    other self-attentions and every cross-attention get ``self_attn_idx=None`` (cross-attention
    becomes :class:`FaceIDAttnProcessor` when ``cfg.condition_on_face_embeds``).  ``cfg`` is the
    reference's ``ModelConfig`` or anything with ``use_adain``, ``train_input`` and
    ``condition_on_face_embeds`` attributes.
    """
    procs = {}
    next_idx = 0
    face_ids = bool(getattr(cfg, "condition_on_face_embeds", False))
    for name in unet.attn_processors.keys():
        is_cross = not name.endswith("attn1.processor")
        if is_cross:
            if face_ids:
                proc = FaceIDAttnProcessor(hidden_size=_hidden_size_for(name, unet.config.block_out_channels),
                                           self_attn_idx=None,
                                           cross_attention_dim=unet.config.cross_attention_dim, embed_dim=512)
            else:
                proc = SharedAttnProcessor(self_attn_idx=None, use_adain=cfg.use_adain, train_input=cfg.train_input)
        elif name.startswith("up_blocks") and "attn1" in name:
            proc = SharedAttnProcessor(self_attn_idx=next_idx, save_self_attentions=save_self_attentions,
                                       use_adain=cfg.use_adain, train_input=cfg.train_input)
            next_idx += 1
        else:
            proc = SharedAttnProcessor(self_attn_idx=None, save_self_attentions=save_self_attentions,
                                       use_adain=cfg.use_adain, train_input=cfg.train_input)
        procs[name] = proc.to(unet.device, dtype=unet.dtype)
    unet.set_attn_processor(procs)
    _lora.invalidate_all(unet)            # (re-)registration starts from freshly folded projection weights
    _lora.install_invalidation_hook(unet)


def set_batch_invariant(unet, enabled: bool = True) -> int:
    """Set ``batch_invariant`` on every :class:`SharedAttnProcessor` and :class:`AttnProcessor` of ``unet`` (the main UNet or the
    reference UNet; call it on both) - the plain attribute, so the processors' constructors stay the reference's.  Returns how
    many processors it reached."""
    n = 0
    for proc in unet.attn_processors.values():
        if isinstance(proc, (SharedAttnProcessor, AttnProcessor)):
            proc.batch_invariant = bool(enabled)
            n += 1
    return n


def register_attention_processor_kv_unet(unet):
    """Put the K/V-capturing :class:`AttnProcessor` on the decoder self-attentions of the frozen
    reference UNet and leave every other processor as it is (attn_processors.py:324-331)."""
    current = unet.attn_processors
    procs = {}
    for name, proc in current.items():
        if name.startswith("up_blocks") and "attn1" in name:
            procs[name] = AttnProcessor().to(unet.device, dtype=unet.dtype)
        else:
            procs[name] = proc
    unet.set_attn_processor(procs)
    _lora.invalidate_all(unet)
    _lora.install_invalidation_hook(unet)


__all__ = ["adain", "AttnProcessor", "FaceIDAttnProcessor", "SharedAttnProcessor",
           "register_attention_processor", "register_attention_processor_kv_unet", "set_batch_invariant"]
