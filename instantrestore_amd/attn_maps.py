"""Host-side helpers around ``ops.attn_rows`` / ``SharedAttnProcessor.attention_rows``: which query tokens the facial
landmarks fall on, and the heat-map picture of a summed row.

The reference does both inside ``get_visualization_image`` (face_replace/training/utils/vis_utils.py:97-108) on the head
mean of the whole ``attention_probs``; here the index list goes IN (``attention_rows_index``) and only the chosen rows are
ever computed.  ``match_coordinates`` / ``match_field`` turn the key indices of ``ops.attn_match`` /
``SharedAttnProcessor.attention_match`` into grid coordinates and displacements."""
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
