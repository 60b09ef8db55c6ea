"""numpy fp64 restatement of the near-duplicate suppression contract (include/crag_dense.h, crag_index_dedupe_async).

Walk a ranked list in order: item i is dropped iff some KEPT item j < i has cos(row_i, row_j) >= threshold; the lowest
such j is its suppressor.  An id that is not stored, the -1 pad and a row with a zero or non-finite norm are kept and
never suppress.  cos = clamp(dot * (1/|i| * 1/|j|), -1, 1), everything in fp64."""
from __future__ import annotations

import numpy as np


def eligible_inv_norm(rows: np.ndarray) -> np.ndarray:
    """1/||row|| in fp64, 0 for a row with a zero or non-finite norm (what the index stores as 'never eligible')."""
    r = np.asarray(rows, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ss = np.sum(r * r, axis=1)
    ok = np.isfinite(ss) & (ss > 0.0)
    inv = np.zeros(len(r), dtype=np.float64)
    inv[ok] = 1.0 / np.sqrt(ss[ok])
    return inv


def dedupe_oracle(stored_ids, rows, ids, threshold: float):
    """stored_ids [n] / rows [n, dim]: the index; ids: one ranked list.  Returns (keep bool [m], dup_of int [m] (-1:
    kept), sim fp64 [m] (NaN: kept), cos fp64 [m, m] (NaN where either item is not eligible))."""
    stored_ids = np.asarray(stored_ids, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    m = ids.size
    inv_all = eligible_inv_norm(rows)
    pos_of = {int(v): i for i, v in enumerate(stored_ids)}
    pos = np.array([pos_of.get(int(v), -1) if int(v) != -1 else -1 for v in ids], dtype=np.int64)
    inv = np.where(pos >= 0, inv_all[np.maximum(pos, 0)], 0.0)
    ok = inv > 0.0
    vec = np.zeros((m, np.asarray(rows).shape[1]), dtype=np.float64)
    vec[ok] = np.asarray(rows, dtype=np.float64)[pos[ok]]
    cos = np.clip((vec @ vec.T) * (inv[:, None] * inv[None, :]), -1.0, 1.0)
    cos[~ok, :] = np.nan
    cos[:, ~ok] = np.nan
    keep = np.ones(m, dtype=bool)
    dup_of = np.full(m, -1, dtype=np.int64)
    sim = np.full(m, np.nan, dtype=np.float64)
    for i in range(m):
        for j in range(i):
            if keep[j] and cos[i, j] >= threshold:   # (NaN compares false)
                keep[i], dup_of[i], sim[i] = False, j, cos[i, j]
                break
    return keep, dup_of, sim, cos
