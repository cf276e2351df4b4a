"""Host-side helpers around ``ops.attn_rows`` / ``SharedAttnProcessor.attention_rows``: which query tokens the facial
landmarks fall on, and the heat-map picture of a summed row.

The reference does both inside ``get_visualization_image`` (face_replace/training/utils/vis_utils.py:97-108) on the head
mean of the whole ``attention_probs``; here the index list goes IN (``attention_rows_index``) and only the chosen rows are
ever computed."""
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
