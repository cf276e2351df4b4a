"""Host-side helpers around ``ops.attn_rows`` / ``SharedAttnProcessor.attention_rows``: which query tokens the facial
landmarks fall on, and the heat-map picture of a summed row.

The reference does both inside ``get_visualization_image`` (face_replace/training/utils/vis_utils.py:97-108) on the head
mean of the whole ``attention_probs``; here the index list goes IN (``attention_rows_index``) and only the chosen rows are
ever computed.  ``match_coordinates`` / ``match_field`` turn the key indices of ``ops.attn_match`` /
``SharedAttnProcessor.attention_match`` into grid coordinates and displacements.  ``coordinate_payload`` / ``image_payload`` build
the per-key payloads of ``ops.attn_transfer`` / ``SharedAttnProcessor.attention_transfer_payload`` and ``soft_match_field`` reads
its sums back as expected positions: the soft form of ``match_field``.  ``received_maps`` / ``keep_from_received`` read the per-key
sums of ``ops.attn_received`` / ``SharedAttnProcessor.attention_received``: pictures per segment, and a ``keep`` mask for
``ops.compact_refs``.  ``topk_coordinates`` / ``match_ambiguity`` / ``topk_coverage`` / ``keep_from_topk`` read the ranks of
``ops.attn_topk`` / ``SharedAttnProcessor.attention_topk``: positions per rank, the ratio test, the share of a segment's attention
its k best keys carry, and the per-query ``keep`` mask.  ``mutual_matches`` / ``mutual_match_field`` / ``keep_from_key_match`` read
``ops.attn_key_match`` / ``SharedAttnProcessor.attention_key_match``: the mutual (cycle) check of ``attn_match``'s pairs, the field
through it, and the max-based ``keep`` mask.  ``token_labels`` samples an integer label picture (a face parsing map) at the token
centres of a layer's grid: the labels ``ops.region_masks`` / the processors' ``region_labels`` take."""
import numpy as np


def landmark_rows(landmarks_xy, side: int, source: int = 512) -> np.ndarray:
    """token index of every landmark on a ``side x side`` token grid: ``(n, 2)`` pixel coordinates ``(x, y)`` of a
    ``source``-pixel image, scaled by ``side / source``, rounded half to even (``np.round``), row-major ``y * side + x``
    (vis_utils.py:97-102).  Several landmarks may share a token (duplicates are kept, in order).  A landmark that lands on or
    past the edge of the grid would index past ``side * side`` tokens (or wrap to another row): ``ValueError``."""
    xy = np.asarray(landmarks_xy, dtype=np.float64).reshape(-1, 2)
    grid = np.round(xy * side / source).astype(np.int64)
    rows = grid[:, 1] * side + grid[:, 0]
    if rows.size and (rows.max() >= side * side or rows.min() < 0):
        raise ValueError(f"landmark token index {int(rows.max())} / {int(rows.min())} outside the {side} x {side} grid "
                         f"(coordinates must round to less than {side} after scaling by {side}/{source})")
    return rows


def landmark_picture(map_row, side: int) -> np.ndarray:
    """``(Lkv,)`` summed row -> ``(side, S * side)`` (vis_utils.py:108; S = Lkv / side**2 = 5: the degraded image and four
    references).  A plain row-major reshape, as the reference does it: each picture row runs through the S segments' tokens
    consecutively."""
    row = map_row.detach().float().cpu().numpy() if hasattr(map_row, "detach") else np.asarray(map_row)
    if row.ndim != 1 or row.size % (side * side):
        raise ValueError(f"expected a ({side * side} * S,) row, got {row.shape}")
    return row.reshape(side, row.size // side)


def _divmod_side(index, side: int):
    """``index`` -> ``(index // side, index % side)`` with negative entries kept as they are (torch tensor on either device,
    or anything NumPy takes)"""
    if hasattr(index, "detach"):
        import torch
        idx = index.detach().long()
        neg = idx < 0
        return (torch.where(neg, idx, torch.div(idx, side, rounding_mode="floor")), torch.where(neg, idx, idx % side))
    idx = np.asarray(index).astype(np.int64)
    neg = idx < 0
    return np.where(neg, idx, idx // side), np.where(neg, idx, idx % side)


def match_coordinates(index, side: int):
    """``index`` of ``ops.attn_match`` / ``SharedAttnProcessor.attention_match`` (any shape; the token inside its segment, row-major
    on a ``side x side`` grid) -> ``(y, x)`` of the matched token, two int64 arrays of ``index``'s shape on its device.  ``-1`` (a row
    index out of range) stays ``-1`` in both.  Index arithmetic only: nothing is read back from the device."""
    return _divmod_side(index, side)


def match_field(index, rows, side: int):
    """the displacement ``(dy, dx)`` from every query token's own place to its match: ``index`` as for
    :func:`match_coordinates`, shaped ``(..., R, S)``; ``rows`` the query tokens the call was given - ``(R,)``, ``(B, R)`` or
    ``None`` / ``"all"`` for ``arange(R)``.  Where ``index`` or the row is negative (out of range) both displacements are 0."""
    y, x = match_coordinates(index, side)
    torch_in = hasattr(index, "detach")
    R = index.shape[-2]
    if rows is None or isinstance(rows, str):
        if torch_in:
            import torch
            rows = torch.arange(R, device=index.device)
        else:
            rows = np.arange(R)
    elif torch_in:
        import torch
        rows = torch.as_tensor(rows).to(index.device)
    qy, qx = _divmod_side(rows, side)
    if qy.ndim == 2 and index.ndim == 4:         # (B, R) against (B, H, R, S)
        qy, qx = qy[:, None], qx[:, None]
    qy, qx = qy[..., None], qx[..., None]         # over the segments
    bad = (y < 0) | (qy < 0)
    zero = 0 * y
    if torch_in:
        import torch
        return torch.where(bad, zero, y - qy), torch.where(bad, zero, x - qx)
    return np.where(bad, zero, y - qy), np.where(bad, zero, x - qx)


def _square_side(length: int, what: str) -> int:
    side = int(round(int(length) ** 0.5))
    if side * side != int(length):
        raise ValueError(f"{what} = {length} is not a square token grid")
    return side


def coordinate_payload(len_self: int, n_refs: int, len_ref: int, include_self: bool, device=None):
    """fp32 ``(1, Lkv, 2)``: the ``(y, x)`` of every key of ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1`` on its OWN
    segment's square grid, row-major - the convention of :func:`match_coordinates`.  As the payload of ``ops.attn_transfer`` it
    gives, per segment, ``sum_j p_j * (y_j, x_j)``: divided by the mass, the expected position inside the segment
    (:func:`soft_match_field`).  One payload serves every batch entry.  A length that is no square: ``ValueError``."""
    import torch
    parts = []
    for length, what, count in ((len_self, "len_self", 1 if include_self else 0), (len_ref, "len_ref", int(n_refs))):
        if count == 0:
            continue
        side = _square_side(length, what)
        idx = torch.arange(int(length), device=device)
        yx = torch.stack([torch.div(idx, side, rounding_mode="floor"), idx % side], dim=-1).to(torch.float32)
        parts += [yx] * count
    if not parts:
        raise ValueError("empty key axis: include_self is False and n_refs is 0")
    return torch.cat(parts, dim=0).unsqueeze(0)


def image_payload(self_image, ref_images, len_self: int, len_ref: int, include_self: bool):
    """fp32 ``(B, Lkv, Cimg)``: pictures laid on the key axis, one token per grid cell.  ``self_image`` ``(B, Cimg, Hp, Wp)`` (ignored
    unless ``include_self``; may then be ``None`` only without it) and ``ref_images`` ``(B, N, Cimg, Hp, Wp)`` (or ``None``: no
    references) are pooled by area to the ``side x side`` token grids of their segments (``side = sqrt(len)``; adaptive average
    pooling, as ``ops.key_bias`` pools a keep map) and flattened row-major.  As the payload of ``ops.attn_transfer`` the sums
    over the reference segments are the attention-warped reference picture.  ``Cimg <= 8`` per call."""
    import torch
    pool = torch.nn.functional.adaptive_avg_pool2d
    parts = []
    if include_self:
        if self_image is None or self_image.dim() != 4:
            raise ValueError("image_payload: include_self needs self_image (B, Cimg, Hp, Wp)")
        side = _square_side(len_self, "len_self")
        parts.append(pool(self_image.to(torch.float32), side).flatten(2).transpose(1, 2))                    # (B, len_self, Cimg)
    if ref_images is not None:
        if ref_images.dim() != 5:
            raise ValueError(f"image_payload: ref_images must be (B, N, Cimg, Hp, Wp), got {tuple(ref_images.shape)}")
        B, N, Ci = ref_images.shape[:3]
        side = _square_side(len_ref, "len_ref")
        r = pool(ref_images.to(torch.float32).flatten(0, 1), side).reshape(B, N, Ci, side * side)
        parts.append(r.permute(0, 1, 3, 2).reshape(B, N * side * side, Ci))                                      # (B, N * len_ref, Cimg)
    if not parts:
        raise ValueError("empty key axis: include_self is False and ref_images is None")
    if len(parts) == 2 and (parts[0].shape[0] != parts[1].shape[0] or parts[0].shape[2] != parts[1].shape[2]):
        raise ValueError(f"image_payload: self_image and ref_images disagree on batch or channels: {tuple(self_image.shape)} vs {tuple(ref_images.shape)}")
    return torch.cat(parts, dim=1).contiguous()


def token_labels(label_image, side: int):
    """per-token class labels from a label picture (a face parsing map): integer ``(B, Hpx, Wpx)`` -> ``(B, side * side)``, or
    ``(B, N, Hpx, Wpx)`` -> ``(B, N * side * side)`` (the references laid end to end, as the key axis lays them), row-major on the
    ``side x side`` token grid - the labels ``ops.region_masks`` takes.  A label is SAMPLED, never averaged: token ``(ty, tx)`` takes
    the pixel at its centre,

        ``py = ((2 * ty + 1) * Hpx) // (2 * side)``,   ``px = ((2 * tx + 1) * Wpx) // (2 * side)``

    (integer floor division; for ``Hpx = k * side`` that is ``ty * k + k // 2``, and for ``Hpx == side`` the picture itself).
    ``Hpx, Wpx >= 1``; a picture smaller than the grid repeats pixels.  Index arithmetic on the picture's device, no sync; the dtype
    is kept."""
    import torch
    img = torch.as_tensor(label_image)
    if img.dim() not in (3, 4) or img.dtype.is_floating_point or img.dtype.is_complex or img.dtype == torch.bool:
        raise ValueError(f"token_labels: label_image must be an integer (B, Hpx, Wpx) or (B, N, Hpx, Wpx) tensor, got {img.dtype} {tuple(img.shape)}")
    side = int(side)
    hpx, wpx = int(img.shape[-2]), int(img.shape[-1])
    if side < 1 or hpx < 1 or wpx < 1:
        raise ValueError(f"token_labels: side {side} and picture {hpx} x {wpx} must be >= 1")
    t = torch.arange(side, device=img.device, dtype=torch.int64)
    py = torch.div((2 * t + 1) * hpx, 2 * side, rounding_mode="floor")
    px = torch.div((2 * t + 1) * wpx, 2 * side, rounding_mode="floor")
    picked = img.index_select(-2, py).index_select(-1, px)          # (..., side, side)
    return picked.reshape(img.shape[0], -1).contiguous()


def token_weights(weight_image, side: int):
    """per-token AdaIN weights from a weight picture (a soft face mask, a confidence map): float or bool ``(B, Hpx, Wpx)`` ->
    fp32 ``(B, side * side)``, or ``(B, N, Hpx, Wpx)`` -> ``(B, N, side * side)`` (one row per reference: the shape
    ``ops.token_stats_weighted`` takes), row-major on the ``side x side`` token grid.  A weight is SAMPLED at the token's centre
    exactly as :func:`token_labels` samples a label - so a 0/1 picture keeps the tokens whose label picture says 1 - never
    averaged: a token is in or out (or carries the picture's own soft value).  Index arithmetic on the picture's device, no sync."""
    import torch
    img = torch.as_tensor(weight_image)
    if img.dim() not in (3, 4) or img.dtype.is_complex:
        raise ValueError(f"token_weights: weight_image must be a real (B, Hpx, Wpx) or (B, N, Hpx, Wpx) tensor, got {img.dtype} {tuple(img.shape)}")
    side = int(side)
    hpx, wpx = int(img.shape[-2]), int(img.shape[-1])
    if side < 1 or hpx < 1 or wpx < 1:
        raise ValueError(f"token_weights: side {side} and picture {hpx} x {wpx} must be >= 1")
    t = torch.arange(side, device=img.device, dtype=torch.int64)
    py = torch.div((2 * t + 1) * hpx, 2 * side, rounding_mode="floor")
    px = torch.div((2 * t + 1) * wpx, 2 * side, rounding_mode="floor")
    picked = img.index_select(-2, py).index_select(-1, px)          # (..., side, side)
    return picked.reshape(*img.shape[:-2], side * side).to(torch.float32).contiguous()


def weights_from_keep(keep):
    """a ``keep`` mask of ``ops.compact_refs`` / ``ref_token_keep`` - bool ``(B, N, len_ref)`` or ``(B, N, S, S)`` - as the fp32
    ``(B, N, len_ref)`` weights of ``ops.token_stats_weighted`` / ``adain_weights``: 1 on a kept token, 0 on a dropped one, so the
    AdaIN statistics are those of the tokens the attention still sees."""
    import torch
    k = torch.as_tensor(keep)
    if k.dim() == 4:
        k = k.reshape(k.shape[0], k.shape[1], -1)
    if k.dim() != 3:
        raise ValueError(f"weights_from_keep: keep must be (B, N, len_ref) or (B, N, S, S), got {tuple(k.shape)}")
    return (k != 0).to(torch.float32).contiguous()


def soft_match_field(sums, mass, rows, side: int):
    """``(sums, mass)`` of ``ops.attn_transfer`` with :func:`coordinate_payload` - ``sums`` ``(..., R, S, 2)``, ``mass`` ``(..., R, S)``,
    torch tensors - -> ``(pos, disp, conf)``: the expected ``(y, x)`` of every (row, segment), ``sums / mass``, fp32
    ``(..., R, S, 2)``; its displacement from the query token's own place on the ``side x side`` grid; and the mass as the
    confidence.  ``rows``: the query tokens the call was given - ``(R,)``, ``(B, R)`` or ``None`` / ``"all"`` for ``arange(R)``.  Where
    the mass is 0 or the row is out of range, position and displacement are 0.  With a one-hot distribution ``pos`` is the key
    of :func:`match_coordinates` and ``disp`` the field of :func:`match_field`."""
    import torch
    R = sums.shape[-3]
    if rows is None or isinstance(rows, str):
        rows = torch.arange(R, device=sums.device)
    else:
        rows = torch.as_tensor(rows).to(sums.device)
    qy, qx = _divmod_side(rows, side)
    if qy.ndim == 2 and sums.ndim == 5:          # (B, R) against (B, H, R, S, 2)
        qy, qx = qy[:, None], qx[:, None]
    own = torch.stack([qy, qx], dim=-1)[..., None, :]                       # (..., R, 1, 2): over the segments
    m = mass.unsqueeze(-1)
    ok = (m > 0) & (own[..., :1] >= 0)
    zero = torch.zeros_like(sums)
    pos = torch.where(ok, sums / torch.where(m > 0, m, torch.ones_like(m)), zero)
    disp = torch.where(ok, pos - own.to(sums.dtype), zero)
    return pos, disp, mass


def _received_axes(recv, len_self: int, n_refs: int, len_ref: int, include_self: bool):
    """the packed key axis of ``recv`` ``(..., Lkv, C)`` checked against the call: ``(offset of reference 0, Lkv)``"""
    off = int(len_self) if include_self else 0
    lkv = off + int(n_refs) * int(len_ref)
    if lkv == 0:
        raise ValueError("empty key axis: include_self is False and n_refs is 0")
    if recv.dim() not in (3, 4) or recv.shape[-2] != lkv:
        raise ValueError(f"recv must be (B, Lkv, C) or (B, H, Lkv, C) with Lkv = {lkv}, got {tuple(recv.shape)}")
    return off, lkv


def received_maps(recv, len_self: int, n_refs: int, len_ref: int, include_self: bool):
    """``recv`` of ``ops.attn_received`` / ``SharedAttnProcessor.attention_received`` - ``(B, Lkv, C)`` or ``(B, H, Lkv, C)`` over
    the packed key axis ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1`` - as per-segment pictures ``(..., S, side, side, C)``,
    ``S = include_self + n_refs``: how much every token of every segment is looked at, on the segment's own square grid, row-major
    (the convention of :func:`match_coordinates`).  A view where the layout allows it.  A segment length that is no square, or a
    self segment and references of different lengths (no common ``side``): ``ValueError``."""
    off, _ = _received_axes(recv, len_self, n_refs, len_ref, include_self)
    lens = ([int(len_self)] if include_self else []) + ([int(len_ref)] if n_refs else [])
    sides = [_square_side(n, what) for n, what in zip(lens, (["len_self"] if include_self else []) + ["len_ref"])]
    if len(set(sides)) != 1:
        raise ValueError(f"len_self = {len_self} and len_ref = {len_ref} are square grids of different sides {sides}: cut recv at "
                         f"{off} and call once per part")
    side, S = sides[0], (1 if include_self else 0) + int(n_refs)
    return recv.reshape(tuple(recv.shape[:-2]) + (S, side, side, recv.shape[-1]))


def keep_from_received(recv, len_self: int, n_refs: int, len_ref: int, include_self: bool, keep_fraction: float):
    """a ``keep`` mask for ``ops.compact_refs`` from the attention the reference tokens received on a warm-up frame: bool
    ``(B, N, len_ref)``, per reference ``True`` on the ``ceil(keep_fraction * len_ref)`` tokens that received most.  The count
    is ``ceil(keep_fraction * len_ref - 1e-9)``, at least 1 and at most ``len_ref``: the ``1e-9`` takes a product that binary
    floating point puts a hair above a whole number back to it (``0.3 * 10`` keeps 3 tokens, not 4).

    ``recv`` as for :func:`received_maps`.  Channel 0 is the score when there are several; a per-head ``recv`` is averaged over its
    heads first.  Ties go to the LOWER token index (a stable descending sort).  Everything stays on ``recv``'s device: no host
    sync beyond what ``torch`` itself does."""
    import math

    import torch
    off, lkv = _received_axes(recv, len_self, n_refs, len_ref, include_self)
    if int(n_refs) < 1:
        raise ValueError("keep_from_received needs n_refs >= 1")
    if not 0.0 < float(keep_fraction) <= 1.0:
        raise ValueError(f"keep_fraction must lie in (0, 1], got {keep_fraction}")
    count = min(int(len_ref), max(1, math.ceil(float(keep_fraction) * int(len_ref) - 1e-9)))
    score = recv[..., 0]
    if score.dim() == 3:
        score = score.mean(dim=1)
    score = score[:, off:lkv].reshape(score.shape[0], int(n_refs), int(len_ref))
    order = torch.sort(-score, dim=-1, stable=True).indices                 # descending, equal scores in ascending token order
    keep = torch.zeros(score.shape, dtype=torch.bool, device=score.device)
    keep.scatter_(-1, order[..., :count], True)
    return keep


def topk_coordinates(index, side: int):
    """``index`` of ``ops.attn_topk`` / ``SharedAttnProcessor.attention_topk`` (``(..., S, k)``; the token inside its segment,
    row-major on a ``side x side`` grid) -> ``(y, x)`` per rank, two int64 arrays of ``index``'s shape on its device.  ``-1`` (a row
    index out of range, or a rank beyond the segment's keys) stays ``-1`` in both.  This is :func:`match_coordinates` on the wider
    shape: index arithmetic only, nothing is read back from the device."""
    return _divmod_side(index, side)


def match_ambiguity(prob):
    """the ratio test on ``prob`` of ``ops.attn_topk`` (``(..., S, k)``, ``k >= 2``): ``prob[..., 1] / prob[..., 0]``, the runner-up
    over the best, in ``[0, 1]`` - 0 for one sharp peak, 1 for two equal ones (a match that may flip between them).  0 where the
    best is 0 or there is no second key (its ``prob`` is 0).  Torch tensor on either device or anything NumPy takes; ``k < 2``:
    ``ValueError``."""
    if prob.shape[-1] < 2:
        raise ValueError(f"match_ambiguity needs the runner-up: k >= 2, got prob of shape {tuple(prob.shape)}")
    best, second = prob[..., 0], prob[..., 1]
    if hasattr(prob, "detach"):
        import torch
        return torch.where(best > 0, second / torch.where(best > 0, best, torch.ones_like(best)), torch.zeros_like(best))
    best, second = np.asarray(best), np.asarray(second)
    return np.where(best > 0, second / np.where(best > 0, best, 1), 0 * best)


def topk_coverage(prob, mass):
    """the share of every segment's attention that its k best keys carry: ``prob.sum(-1) / mass``, clamped to ``[0, 1]``, 0 where
    the mass is 0.  ``prob`` ``(..., S, k)`` of ``ops.attn_topk``; ``mass`` ``(..., S)``: the segment masses of
    ``shared_attention(return_mass=True)`` gathered to the same rows - for a head-mean ``prob`` that mass averaged over the heads.
    Near 1: the attention inside the segment is as sparse as k keys (and ``compact_refs`` may prune hard).  Torch tensors on either
    device or anything NumPy takes."""
    if tuple(prob.shape[:-1]) != tuple(mass.shape):
        raise ValueError(f"topk_coverage: prob {tuple(prob.shape)} needs mass of shape {tuple(prob.shape[:-1])}, got {tuple(mass.shape)}")
    if hasattr(prob, "detach"):
        import torch
        mass = torch.as_tensor(mass).to(device=prob.device, dtype=prob.dtype)
        share = prob.sum(-1) / torch.where(mass > 0, mass, torch.ones_like(mass))
        return torch.where(mass > 0, share, torch.zeros_like(share)).clamp(0, 1)
    prob, mass = np.asarray(prob), np.asarray(mass)
    return np.clip(np.where(mass > 0, prob.sum(-1) / np.where(mass > 0, mass, 1), 0 * mass), 0, 1)


def keep_from_topk(index, n_refs: int, len_ref: int, include_self: bool, min_prob=None, prob=None):
    """a ``keep`` mask for ``ops.compact_refs`` from the ranks of ``ops.attn_topk`` on a warm-up frame: bool ``(B, N, len_ref)``,
    ``True`` on every reference token that is among the k best keys of ANY chosen row (and head) - the per-query counterpart of
    :func:`keep_from_received`, which ranks the tokens by what all rows together give them.  ``index`` ``(B, R, S, k)`` or
    ``(B, H, R, S, k)``, ``S = include_self + n_refs``; the self segment and ``-1`` entries are ignored.  With ``min_prob`` (and the
    ``prob`` of the same call) only ranks with ``prob >= min_prob`` count.  Torch tensors stay on their device; NumPy arrays give a
    NumPy mask."""
    if int(n_refs) < 1:
        raise ValueError("keep_from_topk needs n_refs >= 1")
    first = 1 if include_self else 0
    if len(index.shape) not in (4, 5) or index.shape[-2] != first + int(n_refs):
        raise ValueError(f"index must be (B, R, S, k) or (B, H, R, S, k) with S = {first + int(n_refs)}, got {tuple(index.shape)}")
    if (min_prob is None) != (prob is None):
        raise ValueError("keep_from_topk: min_prob and prob go together")
    if prob is not None and tuple(prob.shape) != tuple(index.shape):
        raise ValueError(f"prob {tuple(prob.shape)} must have index's shape {tuple(index.shape)}")
    B, N, L = index.shape[0], int(n_refs), int(len_ref)
    torch_in = hasattr(index, "detach")
    if torch_in:
        import torch
        idx = index.detach().long()[..., first:, :]
        ok = (idx >= 0) & (idx < L)
        if prob is not None:
            ok = ok & (torch.as_tensor(prob).to(idx.device)[..., first:, :] >= min_prob)
        idx = torch.movedim(idx, -2, 1).reshape(B, N, -1)        # (B, N, every row, head and rank)
        ok = torch.movedim(ok, -2, 1).reshape(B, N, -1)
        # a dropped entry goes to an extra column that is cut off again
        keep = torch.zeros((B, N, L + 1), dtype=torch.bool, device=idx.device)
        keep.scatter_(-1, torch.where(ok, idx, torch.full_like(idx, L)), True)
        return keep[..., :L]
    idx = np.asarray(index).astype(np.int64)[..., first:, :]
    ok = (idx >= 0) & (idx < L)
    if prob is not None:
        ok = ok & (np.asarray(prob)[..., first:, :] >= min_prob)
    idx = np.moveaxis(idx, -2, 1).reshape(B, N, -1)
    ok = np.moveaxis(ok, -2, 1).reshape(B, N, -1)
    keep = np.zeros((B, N, L + 1), dtype=bool)
    np.put_along_axis(keep, np.where(ok, idx, L), True, axis=-1)
    return keep[..., :L]


def _segment_starts(len_self: int, n_refs: int, len_ref: int, include_self: bool):
    """the first column of every segment of ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1`` and the axis' length"""
    off = int(len_self) if include_self else 0
    starts = ([0] if include_self else []) + [off + n * int(len_ref) for n in range(int(n_refs))]
    if not starts:
        raise ValueError("empty key axis: include_self is False and n_refs is 0")
    return starts, off + int(n_refs) * int(len_ref)


def mutual_matches(match_index, key_index, len_self: int, n_refs: int, len_ref: int, include_self: bool, rows=None):
    """the mutual (cycle) check of a correspondence: keep the pair (row ``i``, key ``j``) only if ``j`` is the best key of row
    ``i`` in its segment AND ``i`` is the best row of key ``j``.  ``match_index`` ``(B, R, S)`` or ``(B, H, R, S)`` is the ``index``
    of ``ops.attn_match`` / ``SharedAttnProcessor.attention_match`` (keys counted inside their segments), ``key_index`` ``(B, Lkv)``
    or ``(B, H, Lkv)`` the ``index`` of ``ops.attn_key_match`` / ``SharedAttnProcessor.attention_key_match`` of the SAME call and form
    (query rows, over the packed key axis).  ``rows``: the query tokens ``match_index`` was computed for - ``(R,)``, ``(B, R)`` or
    ``None`` / ``"all"`` for ``arange(R)``.  Returns a bool tensor of ``match_index``'s shape: ``True`` where
    ``key_index[.., col0_s + match_index[.., r, s]] == rows[r]`` with ``col0_s`` the first column of segment ``s``; entries with
    ``match_index < 0`` (or a negative row) are ``False``.  Torch tensors on either device; index arithmetic and one gather, no
    host sync."""
    import torch
    starts, lkv = _segment_starts(len_self, n_refs, len_ref, include_self)
    if match_index.dim() not in (3, 4) or match_index.shape[-1] != len(starts):
        raise ValueError(f"match_index must be (B, R, S) or (B, H, R, S) with S = {len(starts)}, got {tuple(match_index.shape)}")
    if key_index.dim() != match_index.dim() - 1 or key_index.shape[-1] != lkv or tuple(key_index.shape[:-1]) != tuple(match_index.shape[:-2]):
        raise ValueError(f"key_index must be {tuple(match_index.shape[:-2]) + (lkv,)} (the same call and form as match_index), got "
                         f"{tuple(key_index.shape)}")
    dev = match_index.device
    R, S = match_index.shape[-2], match_index.shape[-1]
    if rows is None or isinstance(rows, str):
        rows = torch.arange(R, device=dev)
    else:
        rows = torch.as_tensor(rows).to(dev).long()
    if rows.shape[-1] != R or rows.dim() not in (1, 2):
        raise ValueError(f"rows must be ({R},) or (B, {R}), got {tuple(rows.shape)}")
    if rows.dim() == 2 and match_index.dim() == 4:        # (B, R) against (B, H, R, S)
        rows = rows[:, None]
    rows = rows[..., None]                                 # over the segments
    idx = match_index.detach().long()
    ok = (idx >= 0) & (rows >= 0)
    col = torch.as_tensor(starts, device=dev) + idx.clamp(min=0)
    col = col.clamp(max=lkv - 1)                           # (an index past its segment cannot come from attn_match; never an address)
    back = torch.gather(key_index.detach().long().to(dev), -1, col.reshape(tuple(idx.shape[:-2]) + (R * S,))).reshape(idx.shape)
    return ok & (back == rows)


def mutual_match_field(match_index, key_index, rows, side: int, len_self: int, n_refs: int, len_ref: int, include_self: bool):
    """:func:`match_field` over the pairs that pass :func:`mutual_matches`: ``(dy, dx, mutual)``.  Where the check fails both
    displacements are 0 - exactly as :func:`match_field` marks an entry out of range - and ``mutual`` is ``False`` there: read the
    field through the mask.  Arguments as for the two functions; ``rows`` ``None`` / ``"all"`` for ``arange(R)``."""
    import torch
    rr = None if rows is None or isinstance(rows, str) else rows
    mutual = mutual_matches(match_index, key_index, len_self, n_refs, len_ref, include_self, rows=rr)
    dy, dx = match_field(match_index, rows, side)
    zero = torch.zeros_like(dy)
    return torch.where(mutual, dy, zero), torch.where(mutual, dx, zero), mutual


def keep_from_key_match(prob, len_self: int, n_refs: int, len_ref: int, include_self: bool, *, min_prob=None, keep_fraction=None):
    """a ``keep`` mask for ``ops.compact_refs`` from the column maxima of ``ops.attn_key_match`` on a warm-up frame: bool
    ``(B, N, len_ref)``.  The max-based counterpart of :func:`keep_from_received`: that one keeps tokens that collect a lot of
    attention in total, this one tokens that AT LEAST ONE query token looks at strongly - which a small but decisive feature (an eye
    corner) survives.  ``prob`` ``(B, Lkv)`` (the head-mean form) or ``(B, H, Lkv)`` (per head: reduced by a maximum over the
    heads).  Exactly one rule: ``min_prob`` - ``True`` where the score is ``>= min_prob``; ``keep_fraction`` - per reference the
    ``ceil(keep_fraction * len_ref - 1e-9)`` tokens with the largest score, at least 1 and at most ``len_ref``, ties to the LOWER
    token index (the count and the order of :func:`keep_from_received`).  Everything stays on ``prob``'s device."""
    import math

    import torch
    starts, lkv = _segment_starts(len_self, n_refs, len_ref, include_self)
    if int(n_refs) < 1:
        raise ValueError("keep_from_key_match needs n_refs >= 1")
    if prob.dim() not in (2, 3) or prob.shape[-1] != lkv:
        raise ValueError(f"prob must be (B, Lkv) or (B, H, Lkv) with Lkv = {lkv}, got {tuple(prob.shape)}")
    if (min_prob is None) == (keep_fraction is None):
        raise ValueError("keep_from_key_match takes exactly one of min_prob and keep_fraction")
    score = prob.amax(dim=1) if prob.dim() == 3 else prob
    off = lkv - int(n_refs) * int(len_ref)
    score = score[:, off:lkv].reshape(score.shape[0], int(n_refs), int(len_ref))
    if min_prob is not None:
        return score >= min_prob
    if not 0.0 < float(keep_fraction) <= 1.0:
        raise ValueError(f"keep_fraction must lie in (0, 1], got {keep_fraction}")
    count = min(int(len_ref), max(1, math.ceil(float(keep_fraction) * int(len_ref) - 1e-9)))
    order = torch.sort(-score, dim=-1, stable=True).indices                 # descending, equal scores in ascending token order
    keep = torch.zeros(score.shape, dtype=torch.bool, device=score.device)
    keep.scatter_(-1, order[..., :count], True)
    return keep
