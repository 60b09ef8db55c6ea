"""numpy fp64 restatement of the MMR contract (include/crag_dense.h, crag_index_mmr_async).

A slot is a candidate when its id is not -1, its rel is finite and no earlier slot holds the same id.  A candidate is
comparable when its id is stored with a finite non-zero norm.  k times, while candidates remain, the candidate with the
largest value = lam * rel - (1 - lam) * pen is picked, equal values going to the lower id; pen is 0 until a picked comparable
item meets a comparable one: the first cosine sets it, later ones raise it (max).  Everything in fp64; lam and 1 - lam are
the fp32 numbers the C ABI computes with (lam rounded to fp32, mu = 1.0f - lam)."""
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


def pair_cosines(stored_ids, rows, ids) -> np.ndarray:
    """fp64 [m, m] cosines of the rows behind one list of ids; NaN where either item is not comparable."""
    stored_ids = np.asarray(stored_ids, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    m = ids.size
    rows = np.asarray(rows)
    inv_all = eligible_inv_norm(rows) if len(rows) else np.zeros(0)
    pos_of = {int(v): i for i, v in enumerate(stored_ids)}
    pos = np.array([pos_of.get(int(v), -1) if int(v) != -1 else -1 for v in ids], dtype=np.int64)
    inv = np.where(pos >= 0, inv_all[np.maximum(pos, 0)], 0.0) if len(rows) else np.zeros(m)
    ok = inv > 0.0
    vec = np.zeros((m, rows.shape[1]), dtype=np.float64)
    vec[ok] = rows.astype(np.float64)[pos[ok]]
    with np.errstate(invalid="ignore"):
        cos = np.clip((vec @ vec.T) * (inv[:, None] * inv[None, :]), -1.0, 1.0)
    cos[~ok, :] = np.nan
    cos[:, ~ok] = np.nan
    return cos


def candidate_slots(rel, ids) -> np.ndarray:
    rel = np.asarray(rel, dtype=np.float64).reshape(-1)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    out = np.zeros(ids.size, dtype=bool)
    for i in range(ids.size):
        out[i] = ids[i] != -1 and np.isfinite(rel[i]) and not np.any(ids[:i] == ids[i])
    return out


def mmr_oracle(rel, cos, lam: float, k: int, ids):
    """rel [m], cos [m, m] (NaN: not comparable), ids [m].  Returns (slots int64 [count], values fp64 [count], gaps fp64
    [count]): per step the winning value minus the runner-up's (inf when one candidate is left)."""
    rel = np.asarray(rel, dtype=np.float64).reshape(-1)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    cos = np.asarray(cos, dtype=np.float64)
    lam64 = float(np.float32(lam))
    mu64 = float(np.float32(1.0) - np.float32(lam))
    cand = candidate_slots(rel, ids)
    left = cand.copy()
    pen = np.zeros(ids.size, dtype=np.float64)
    met = np.zeros(ids.size, dtype=bool)
    slots, values, gaps = [], [], []
    for _ in range(int(k)):
        live = np.flatnonzero(left)
        if live.size == 0:
            break
        value = lam64 * rel - mu64 * pen
        order = sorted(live.tolist(), key=lambda i: (-value[i], int(ids[i])))
        pick = order[0]
        slots.append(pick)
        values.append(value[pick])
        gaps.append(value[pick] - value[order[1]] if len(order) > 1 else np.inf)
        left[pick] = False
        for i in np.flatnonzero(cand):
            c = cos[pick, i]
            if not np.isnan(c):
                pen[i] = max(pen[i], c) if met[i] else c
                met[i] = True
    return np.asarray(slots, dtype=np.int64), np.asarray(values, dtype=np.float64), np.asarray(gaps, dtype=np.float64)


def crafted(seed: int, dim: int = 1024):
    """8 clusters x 5 members, each cluster in its own 128-dim band (cross-cluster cosines exactly 0, in-cluster ~0.98 to
    0.997), row norms in [0.2, 5], shuffled; rel a shuffled grid spaced 1/64 downward from 0.9.  Returns (rows fp32
    [40, dim], ids int64 [40] ascending, rel fp32 [40])."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((40, dim), dtype=np.float64)
    for c in range(8):
        base = rng.standard_normal(128)
        base /= np.linalg.norm(base)
        for m in range(5):
            e = rng.standard_normal(128)
            e /= np.linalg.norm(e)
            rows[c * 5 + m, c * 128:(c + 1) * 128] = (base + rng.uniform(0.05, 0.14) * e) * rng.uniform(0.2, 5.0)
    rows = rows[rng.permutation(40)].astype(np.float32)
    ids = 100 + 7 * np.arange(40, dtype=np.int64)
    rel = (0.9 - np.arange(40) / 64.0)[rng.permutation(40)].astype(np.float32)
    return rows, ids, rel


def crafted_query(rows: np.ndarray, seed: int) -> np.ndarray:
    """A query for the rows of `crafted`: the least-norm q whose product with every unit row is (a weight of the row's
    cluster, 0.9 downward in steps of 0.09) + (0.012 x the member's shuffled number), so that the cosines to q differ by
    ~0.04 between clusters and ~0.005 inside one."""
    rng = np.random.default_rng(seed)
    r = np.asarray(rows, dtype=np.float64)
    unit = r / np.linalg.norm(r, axis=1, keepdims=True)
    band = np.argmax(np.abs(r).reshape(len(r), 8, -1).sum(axis=2), axis=1)
    weight = 0.9 - 0.09 * rng.permutation(8)
    target = np.empty(len(r))
    for c in range(8):
        members = np.flatnonzero(band == c)
        target[members] = weight[c] + 0.012 * rng.permutation(members.size)
    return np.linalg.lstsq(unit, target, rcond=None)[0].astype(np.float32)
