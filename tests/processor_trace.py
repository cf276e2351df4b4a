"""Call traces of ``SharedAttnProcessor.forward``: a recorder that stands in for ``attn_processors._ops`` and the list of cases.

The recorder computes nothing.  Every entry point notes its name and, for each positional and keyword argument, ``None``, dtype and
shape (a tensor), the value (bool / int / str), the value rounded to 6 places (a float) or the type's name (anything else), and
returns zeros or ones of the documented shape; ``key_bias`` and ``region_masks`` are the real plain-torch functions.  What a case
leaves behind - the calls in order, how it ended, the processor's result attributes - is what ``tests/golden/processor_trace.json``
holds (``tests/golden/make_processor_trace.py`` writes it, ``tests/test_processor_trace_cpu.py`` compares)."""
import importlib

import torch

B, H, L, N, C = 2, 2, 16, 3, 128
RESULTS = ("attention_mass", "attention_rows", "attention_match", "attention_transfer", "attention_received", "attention_topk",
           "attention_key_match", "attention_probs")


def describe(v):
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return round(v, 6)
    if isinstance(v, torch.Tensor):
        return f"{str(v.dtype)[6:]}{list(v.shape)}"
    if isinstance(v, (tuple, list)):
        return [describe(x) for x in v]
    if hasattr(v, "ptrs") and hasattr(v, "row_stride"):
        return f"table:{str(v.dtype)[6:]}{list(v.shape)}"
    return type(v).__name__


class Partials:
    """stands for ``ops.ColumnStats``: what the q/k/v GEMM's statistics tail leaves behind"""


class RefStats:
    """stands for ``ops.RefStatsPartials``: content statistics that arrive as partials, finished on demand"""

    def __init__(self):
        self.part, self.valid = Partials(), torch.full((B,), N, dtype=torch.int32)

    def finished(self):
        return torch.zeros(B, N, H, 64), torch.ones(B, N, H, 64)

    def sync_to_current(self):
        pass

    def record_stream(self, stream):
        pass


def _pair(x, heads, *lead):
    shape = (x.shape[0], *lead, x.shape[1], heads, 64)
    return torch.zeros(shape), torch.ones(shape)


class Recorder:
    HEAD_DIM = 64
    ADAIN_EPS = 1e-5
    STATS_MAX_CHUNKS = 64

    def __init__(self, ops, own_gemm=False):
        self._real, self.own_gemm, self.calls = ops, own_gemm, []

    def _rec(self, name, args, kw):
        self.calls.append([name, [describe(a) for a in args], {k: describe(v) for k, v in sorted(kw.items())}])

    # predicates: not launches, not recorded
    def linear_supported(self, x, w, b):
        return self.own_gemm

    def tuning_supports_prescaled_q(self):
        return True

    def linear_stats_rows(self, rows, n, k, bias):
        return 4

    def linear(self, x, w, bias=None, **kw):
        self._rec("linear", (x, w, bias), kw)
        y = torch.zeros(*x.shape[:-1], w.shape[0], dtype=w.dtype)
        return (y, Partials()) if "stats" in kw else y

    def key_bias(self, *a, **kw):
        self._rec("key_bias", a, kw)
        return self._real.key_bias(*a, **kw)

    def region_masks(self, *a, **kw):
        self._rec("region_masks", a, kw)
        return self._real.region_masks(*a, **kw)

    def token_stats(self, x, **kw):
        self._rec("token_stats", (x,), kw)
        return _pair(x, kw["heads"])

    def token_stats_weighted(self, x, **kw):
        self._rec("token_stats_weighted", (x,), kw)
        return _pair(x, kw["heads"])

    def token_stats_regions(self, x, labels, **kw):
        self._rec("token_stats_regions", (x, labels), kw)
        return _pair(x, kw["heads"], kw["n_regions"]) + (torch.full((x.shape[0], kw["n_regions"], x.shape[1]), 100.0),)

    def adain_stats(self, v, ref_v, **kw):
        self._rec("adain_stats", (v, ref_v), kw)
        return _pair(ref_v, kw["heads"])[::-1]

    def adain_stats_cached(self, v, mean, std, **kw):
        self._rec("adain_stats_cached", (v, mean, std), kw)
        return torch.ones_like(mean), torch.zeros_like(mean)

    def adain_affine(self, style, content, **kw):
        self._rec("adain_affine", (style, content), kw)
        return torch.ones_like(content[0]), torch.zeros_like(content[0])

    def adain_affine_from_partials(self, style, batch, len_self, n_refs, len_ref, **kw):
        self._rec("adain_affine_from_partials", (style, batch, len_self, n_refs, len_ref), kw)
        return torch.ones(batch, n_refs, H, 64), torch.zeros(batch, n_refs, H, 64)

    def adain_affine_regions(self, style, content, style_global, content_global, **kw):
        self._rec("adain_affine_regions", (style, content, style_global, content_global), kw)
        b, r, n, h, d = content[0].shape
        return torch.ones(b, n, r + 1, h, d), torch.zeros(b, n, r + 1, h, d)

    def adain_apply(self, x, a, b, **kw):
        self._rec("adain_apply", (x, a, b), kw)
        return torch.zeros_like(x)

    def adain_apply_regions(self, x, labels, a, b, **kw):
        self._rec("adain_apply_regions", (x, labels, a, b), kw)
        return torch.zeros_like(x)

    def shared_attention(self, q, k_self, v_self, ref_k=None, ref_v=None, **kw):
        self._rec("shared_attention", (q, k_self, v_self, ref_k, ref_v), kw)
        res = [torch.zeros_like(q)]
        if kw.get("return_lse"):
            res.append(torch.zeros(q.shape[0], kw["heads"], q.shape[1]))
        if kw.get("return_mass"):
            res.append(torch.zeros(q.shape[0], kw["heads"], q.shape[1], self._axes(k_self, ref_k, kw)[1]))
        return res[0] if len(res) == 1 else tuple(res)

    @staticmethod
    def _axes(k_self, ref_k, kw):
        own = 1 if kw.get("include_self", True) else 0
        lkv = own * k_self.shape[1] + (ref_k.shape[1] * ref_k.shape[2] if ref_k is not None else 0)
        return lkv, own + (ref_k.shape[1] if ref_k is not None else 0)

    @staticmethod
    def _lead(q, kw, rows="all"):
        lead = (q.shape[0],) + ((kw["heads"],) if kw.get("reduce", "none") == "none" else ())
        return lead if rows == "all" else lead + (q.shape[1] if rows is None else torch.as_tensor(rows).shape[-1],)

    def attn_probs(self, q, k_self, ref_k, lse, **kw):
        self._rec("attn_probs", (q, k_self, ref_k, lse), kw)
        return torch.zeros(q.shape[0], kw["heads"], q.shape[1], self._axes(k_self, ref_k, kw)[0], dtype=q.dtype)

    def attn_rows(self, q, k_self, ref_k, lse, rows, **kw):
        self._rec("attn_rows", (q, k_self, ref_k, lse, rows), kw)
        lkv = self._axes(k_self, ref_k, kw)[0]
        if kw.get("reduce", "none") == "map":
            return torch.zeros(q.shape[0], lkv)
        return torch.zeros(*self._lead(q, kw, rows), lkv, dtype=q.dtype if kw.get("reduce", "none") == "none" else torch.float32)

    def attn_match(self, q, k_self, ref_k, lse, rows=None, **kw):
        self._rec("attn_match", (q, k_self, ref_k, lse, rows), kw)
        shape = self._lead(q, kw, rows) + (self._axes(k_self, ref_k, kw)[1],)
        return torch.zeros(shape, dtype=torch.int32), torch.zeros(shape)

    def attn_topk(self, q, k_self, ref_k, lse, rows=None, **kw):
        self._rec("attn_topk", (q, k_self, ref_k, lse, rows), kw)
        shape = self._lead(q, kw, rows) + (self._axes(k_self, ref_k, kw)[1], kw["k"])
        return torch.zeros(shape, dtype=torch.int32), torch.zeros(shape)

    def attn_transfer(self, q, k_self, ref_k, lse, payload, rows=None, **kw):
        self._rec("attn_transfer", (q, k_self, ref_k, lse, payload, rows), kw)
        shape = self._lead(q, kw, rows) + (self._axes(k_self, ref_k, kw)[1],)
        return torch.zeros(shape + (payload.shape[-1],)), torch.zeros(shape)

    def attn_received(self, q, k_self, ref_k, lse, weights=None, **kw):
        self._rec("attn_received", (q, k_self, ref_k, lse, weights), kw)
        nch = 1 if weights is None or weights.dim() == 1 else weights.shape[-1]
        return torch.zeros(*self._lead(q, kw), self._axes(k_self, ref_k, kw)[0], nch)

    def attn_key_match(self, q, k_self, ref_k, lse, **kw):
        self._rec("attn_key_match", (q, k_self, ref_k, lse), kw)
        shape = self._lead(q, kw) + (self._axes(k_self, ref_k, kw)[0],)
        return torch.zeros(shape, dtype=torch.int32), torch.zeros(shape)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def cases():
    """name -> case, built afresh at every call (the processors' caches go by tensor identity).  A case: ``layer`` (constructor
    arguments), ``attrs`` (set on the processor), ``kw`` (handed to the call), ``own`` (the own-GEMM switch), ``length`` (tokens of
    this image and of a reference), ``table`` (references as ``RefKVTable``), ``repeat`` (calls with the same kwargs)"""
    lkv = L + N * L
    stats = lambda: [(torch.zeros(B, N, H, 64), torch.ones(B, N, H, 64))]
    lab_q, lab_r = (torch.arange(L) % 2).expand(B, L).contiguous(), (torch.arange(L) % 2).expand(B, N, L).contiguous()
    labels = lambda: (lab_q.clone(), lab_r.clone())
    allow = lambda: torch.eye(2, dtype=torch.bool)
    lens = lambda: [torch.full((B, N), L - 3, dtype=torch.int32)]
    keep = lambda: torch.arange(L).expand(B, N, L) % 3 != 0
    rows = lambda: torch.tensor([0, 3, 15])
    every = lambda: dict(save_self_attentions=True, save_attention_mass=True, attention_rows_index=rows(), attention_match_index="all",
                         attention_topk_index="all", attention_transfer_payload=torch.zeros(lkv, 2), attention_received_weights="ones",
                         attention_key_match_reduce="head_mean")
    # the seven switches of the read-outs, each as the smallest setting that turns it on
    switches = {"probs": dict(save_self_attentions=True), "rows": dict(attention_rows_index=rows()),
                "match": dict(attention_match_index="all"), "transfer": dict(attention_transfer_payload=torch.zeros(lkv, 2)),
                "received": dict(attention_received_weights="ones"), "topk": dict(attention_topk_index="all"),
                "key_match": dict(attention_key_match_reduce="none")}
    adain = dict(use_adain=True)
    mass = dict(save_attention_mass=True)
    c = {}
    # -- calls that succeed
    c["plain"] = {}
    c["plain_no_train_input"] = dict(layer=dict(train_input=False))
    c["unshared_every_kwarg"] = dict(layer=dict(self_attn_idx=None, use_adain=True), attrs=dict(every(), attention_transfer_payload=torch.zeros(L, 2)), kw=dict(
        ref_events=[None], ref_stats=stats(), ref_valid=torch.full((B,), N, dtype=torch.int32), ref_weights=torch.ones(B, N),
        ref_token_keep=keep(), ref_lens=lens(), region_labels=labels(), region_allow=allow(), adain_weights=(torch.ones(B, L), None),
        adain_regions=labels(), adain_n_regions=2, adain_region_min_tokens=2))
    c["unshared_mask"] = dict(layer=dict(self_attn_idx=None), kw=dict(attention_mask=torch.zeros(B, 1, L)))
    c["every_readout"] = dict(attrs=every())
    c["every_readout_no_train_input"] = dict(layer=dict(train_input=False), attrs=dict(every(), attention_transfer_payload=torch.zeros(N * L, 2)))
    c["every_readout_per_head"] = dict(attrs=dict(every(), attention_rows_reduce="none", attention_match_reduce="none",
                                                  attention_transfer_reduce="none", attention_received_reduce="none",
                                                  attention_topk_reduce="none", attention_key_match_reduce="none", attention_topk_k=2))
    c["mass_alone"] = dict(attrs=mass)
    c["probs_alone"] = dict(attrs=dict(save_self_attentions=True))
    c["probs_and_mass"] = dict(attrs=dict(mass, save_self_attentions=True))
    c["rows_tensor"] = dict(attrs=dict(attention_rows_index=rows()))
    c["rows_per_entry_map"] = dict(attrs=dict(attention_rows_index=torch.tensor([[0, 1], [2, 3]]), attention_rows_reduce="map"))
    c["match_tensor"] = dict(attrs=dict(attention_match_index=rows()))
    c["match_all"] = dict(attrs=dict(attention_match_index="all", attention_match_reduce="none"))
    c["transfer_every_row"] = dict(attrs=dict(attention_transfer_payload=torch.zeros(B, lkv, 3)))
    c["transfer_tensor"] = dict(attrs=dict(attention_transfer_payload=torch.zeros(lkv, 2), attention_transfer_index=rows()))
    c["transfer_all"] = dict(attrs=dict(attention_transfer_payload=torch.zeros(lkv, 2), attention_transfer_index="all"))
    c["received_tensor"] = dict(attrs=dict(attention_received_weights=torch.ones(L, 2)))
    c["received_ones"] = dict(attrs=dict(attention_received_weights="ones", attention_received_reduce="none"))
    c["topk_tensor"] = dict(attrs=dict(attention_topk_index=rows(), attention_topk_k=2))
    c["topk_all"] = dict(attrs=dict(attention_topk_index="all"))
    c["key_match_head_mean"] = dict(attrs=dict(attention_key_match_reduce="head_mean"))
    c["key_match_per_head"] = dict(attrs=dict(attention_key_match_reduce="none"))
    c["own_gemm"] = dict(own=True)
    c["own_gemm_every_readout"] = dict(own=True, attrs=every())
    c["own_gemm_adain_dense"] = dict(own=True, layer=adain)
    c["own_gemm_adain_tuple_stats"] = dict(own=True, layer=adain, kw=dict(ref_stats=stats()))
    c["own_gemm_adain_partials"] = dict(own=True, layer=adain, kw=dict(ref_stats=[RefStats()]))
    c["own_gemm_adain_weighted"] = dict(own=True, layer=adain, kw=dict(ref_stats=stats(), adain_weights=(torch.ones(B, L), None)))
    c["batch_invariant"] = dict(own=True, attrs=dict(batch_invariant=True))
    c["batch_invariant_every_readout"] = dict(own=True, attrs=dict(every(), batch_invariant=True))
    c["batch_invariant_adain_partials"] = dict(own=True, layer=adain, attrs=dict(batch_invariant=True), kw=dict(ref_stats=[RefStats()]))
    c["adain_dense"] = dict(layer=adain)
    c["adain_cached"] = dict(layer=adain, kw=dict(ref_stats=stats()))
    c["adain_finished"] = dict(layer=adain, kw=dict(ref_stats=[RefStats()]))
    c["adain_table_cached"] = dict(layer=adain, table=True, kw=dict(ref_stats=stats()))
    c["adain_short_reference"] = dict(layer=adain, length=4, kw=dict(ref_valid=torch.full((B,), N, dtype=torch.int32)))
    c["adain_dense_valid"] = dict(layer=adain, kw=dict(ref_valid=torch.full((B,), N, dtype=torch.int32)))
    c["adain_weights_stats"] = dict(layer=adain, kw=dict(ref_stats=stats(), adain_weights=(torch.ones(B, L), torch.ones(B, N, L))))
    c["adain_weights_finished"] = dict(layer=adain, kw=dict(ref_stats=[RefStats()], adain_weights=(torch.ones(B, L), None)))
    c["adain_weights_dense"] = dict(layer=adain, kw=dict(adain_weights=(torch.ones(B, L) > 0, torch.ones(B, N, L))))
    c["adain_weights_no_self_side"] = dict(layer=adain, kw=dict(adain_weights=(None, torch.ones(B, N, L))))
    c["adain_weights_pictures"] = dict(layer=adain, kw=dict(adain_weights=(torch.ones(B, 8, 8), torch.ones(B, N, 64))))
    c["adain_weights_unused"] = dict(kw=dict(adain_weights=(torch.ones(B, L), None)))
    c["adain_regions"] = dict(layer=adain, kw=dict(adain_regions=labels(), adain_n_regions=2, ref_valid=torch.full((B,), N, dtype=torch.int32)))
    c["adain_regions_min_tokens"] = dict(layer=adain, kw=dict(adain_regions=labels(), adain_n_regions=2, adain_region_min_tokens=3,
                                                              ref_stats=stats()))
    c["adain_regions_pictures"] = dict(layer=adain, kw=dict(adain_regions=(torch.zeros(B, 8, 8, dtype=torch.int64),
                                                                           torch.zeros(B, N, 64, dtype=torch.int64)), adain_n_regions=1))
    for name, mask in (("rows", torch.zeros(B, lkv)), ("broadcast", torch.zeros(B, 1, lkv)), ("per_head", torch.zeros(B * H, 1, lkv))):
        c[f"mask_{name}"] = dict(attrs=mass, kw=dict(attention_mask=mask))
    c["ref_weights"] = dict(attrs=mass, kw=dict(ref_weights=torch.ones(B, N)))
    c["ref_token_keep"] = dict(attrs=mass, kw=dict(ref_token_keep=keep()))
    c["mask_and_ref_weights"] = dict(attrs=mass, kw=dict(attention_mask=torch.zeros(B * H, 1, lkv), ref_weights=torch.ones(B, N)))
    c["bias_adain"] = dict(layer=adain, attrs=mass, kw=dict(ref_weights=torch.ones(B, N), ref_token_keep=keep()))
    c["regions"] = dict(attrs=mass, kw=dict(region_labels=labels(), region_allow=allow()))
    c["regions_no_train_input"] = dict(layer=dict(train_input=False), kw=dict(region_labels=labels(), region_allow=allow()))
    c["regions_pictures"] = dict(kw=dict(region_labels=(torch.zeros(B, 8, 8, dtype=torch.int64), torch.zeros(B, N, 64, dtype=torch.int64)),
                                         region_allow=allow()))
    c["regions_valid"] = dict(kw=dict(region_labels=labels(), region_allow=allow(), ref_valid=torch.full((B,), N, dtype=torch.int32)))
    c["regions_adain_regions"] = dict(layer=adain, kw=dict(region_labels=labels(), region_allow=allow(), adain_regions=labels(), adain_n_regions=2))
    c["ref_lens"] = dict(attrs=mass, kw=dict(ref_lens=lens()))
    c["ref_lens_adain_stats"] = dict(layer=adain, kw=dict(ref_lens=lens(), ref_stats=stats()))
    c["ref_lens_adain_weights"] = dict(layer=adain, kw=dict(ref_lens=lens(), ref_stats=stats(), adain_weights=(torch.ones(B, L), None)))
    c["ref_lens_none_here"] = dict(attrs=dict(save_self_attentions=True), kw=dict(ref_lens=[None], ref_valid=torch.full((B,), N, dtype=torch.int32)))
    c["twice_bias"] = dict(repeat=2, kw=dict(ref_weights=torch.ones(B, N), ref_token_keep=keep()))
    c["twice_regions"] = dict(repeat=2, kw=dict(region_labels=labels(), region_allow=allow()))
    c["twice_adain_inputs"] = dict(repeat=2, layer=adain, kw=dict(adain_weights=(torch.ones(B, 8, 8), torch.ones(B, N, 8, 8))))
    # -- calls that are refused: each of the three rules with each of the seven switches
    for name, attrs in switches.items():
        c[f"refused_regions_x_{name}"] = dict(attrs=dict(attrs), kw=dict(region_labels=labels(), region_allow=allow()))
        c[f"refused_ref_lens_x_{name}"] = dict(attrs=dict(attrs), kw=dict(ref_lens=lens()))
        c[f"refused_bias_x_{name}"] = dict(attrs=dict(attrs), kw=dict(ref_weights=torch.ones(B, N)))
    c["refused_mask_x_probs_unshared"] = dict(layer=dict(self_attn_idx=None, save_self_attentions=True), kw=dict(attention_mask=torch.zeros(B, L)))
    c["refused_adain_regions_no_count"] = dict(layer=adain, kw=dict(adain_regions=labels()))
    c["refused_adain_regions_x_weights"] = dict(layer=adain, kw=dict(adain_regions=labels(), adain_n_regions=2, adain_weights=(torch.ones(B, L), None)))
    c["refused_adain_regions_x_ref_lens"] = dict(layer=adain, kw=dict(adain_regions=labels(), adain_n_regions=2, ref_lens=lens(), ref_stats=stats()))
    c["refused_adain_regions_x_table"] = dict(layer=adain, table=True, kw=dict(adain_regions=labels(), adain_n_regions=2, ref_stats=stats()))
    c["refused_ref_lens_x_valid"] = dict(kw=dict(ref_lens=lens(), ref_valid=torch.full((B,), N, dtype=torch.int32)))
    c["refused_ref_lens_x_ref_weights"] = dict(kw=dict(ref_lens=lens(), ref_weights=torch.ones(B, N)))
    c["refused_ref_lens_x_mask"] = dict(kw=dict(ref_lens=lens(), attention_mask=torch.zeros(B, lkv)))
    c["refused_ref_lens_adain_no_stats"] = dict(layer=adain, kw=dict(ref_lens=lens()))
    c["refused_regions_x_ref_token_keep"] = dict(kw=dict(region_labels=labels(), region_allow=allow(), ref_token_keep=keep()))
    c["refused_regions_x_ref_lens"] = dict(kw=dict(region_labels=labels(), region_allow=allow(), ref_lens=lens()))
    c["refused_regions_no_allow"] = dict(kw=dict(region_labels=labels()))
    c["refused_match_sentinel"] = dict(attrs=dict(attention_match_index="every"))
    c["refused_transfer_sentinel"] = dict(attrs=dict(attention_transfer_payload=torch.zeros(lkv, 2), attention_transfer_index="every"))
    c["refused_received_sentinel"] = dict(attrs=dict(attention_received_weights="all"))
    c["refused_topk_sentinel"] = dict(attrs=dict(attention_topk_index="ones"))
    c["refused_key_match_reduce"] = dict(attrs=dict(attention_key_match_reduce="map"))
    c["refused_region_labels_no_pair"] = dict(kw=dict(region_labels=lab_q.clone(), region_allow=allow()))
    c["refused_adain_weights_no_pair"] = dict(layer=adain, kw=dict(adain_weights=torch.ones(B, L)))
    c["refused_adain_table_no_stats"] = dict(layer=adain, table=True)
    c["refused_adain_weights_table_no_stats"] = dict(layer=adain, table=True, kw=dict(adain_weights=(torch.ones(B, L), None)))
    c["refused_adain_short_table"] = dict(layer=adain, table=True, length=4, kw=dict(ref_stats=stats()))
    return c


def run_case(ap, case):
    """one case against the processors module ``ap`` -> ``{"calls", "end", "out", "left"}``"""
    pkg = ap.__name__.rpartition(".")[0]
    ops = importlib.import_module(pkg + ".ops")
    attention = importlib.import_module(pkg + ".attention")
    rec = Recorder(ops, own_gemm=bool(case.get("own")))
    for cache in (ap._BIAS_ROWS, ap._REGION_PAIRS, ap._ADAIN_WEIGHTS, ap._ADAIN_REGION_LABELS):
        cache.clear()
    layer = dict(self_attn_idx=0)
    layer.update(case.get("layer", {}))
    proc = ap.SharedAttnProcessor(**layer)
    for name, value in case.get("attrs", {}).items():
        setattr(proc, name, value)
    attn = attention.Attention(query_dim=C, heads=H, dim_head=64, processor=proc)
    length = case.get("length", L)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, length, C, generator=g)
    rk, rv = torch.randn(B, N, length, C, generator=g), torch.randn(B, N, length, C, generator=g)
    if case.get("table"):
        rk, rv = (ops.RefKVTable.from_tensors([[t[b, n] for n in range(N)] for b in range(B)]) for t in (rk, rv))
    kw = dict(ref_keys=[rk], ref_values=[rv])
    kw.update(case.get("kw", {}))
    saved, ap._ops = ap._ops, rec
    out, end = None, "ok"
    try:
        with torch.no_grad():
            for _ in range(case.get("repeat", 1)):
                out = attn(x, **kw)
    except Exception as e:      # a refusal: its type and text are the result
        out, end = None, [type(e).__name__, str(e)]
    finally:
        ap._ops = saved
    return {"calls": rec.calls, "end": end, "out": describe(out), "left": {n: describe(getattr(proc, n, None)) for n in RESULTS}}


def run_all(ap):
    return {name: run_case(ap, case) for name, case in cases().items()}
