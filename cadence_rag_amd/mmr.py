"""Maximal marginal relevance over one ranked list: the rule of crag_index_mmr_async (include/crag_dense.h) in numpy, and
the record the dense lane takes its MMR settings in.

`mmr_host` is the GPU walk operation for operation: np.float32 mul / mul / sub round where the kernel rounds, so with the
kernel's own pair cosines it reproduces the kernel's picks and value bits exactly; with any other matrix of cosines it is
the definition of the rule.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np

MMR_MAX_WIDTH = 256   # CRAG_MMR_MAX_WIDTH


@dataclass(frozen=True)
class MmrParams:
    """MMR on a dense lane (DenseTable.fetch_dense): `lam` in [0, 1] weighs relevance against redundancy (1 = the plain
    ranking), `fetch` is how many rows the lane fetches to pick its limit from (0: min(4 * limit, 256))."""
    lam: float
    fetch: int = 0

    def __post_init__(self) -> None:
        if not 0.0 <= float(self.lam) <= 1.0:   # (NaN fails both)
            raise ValueError(f"lam must be finite, in [0, 1] (got {self.lam})")
        if int(self.fetch) < 0:
            raise ValueError(f"fetch must be >= 0 (got {self.fetch})")

    def fetch_for(self, limit: int) -> int:
        """Rows to fetch for `limit` picks: at least `limit`, at most MMR_MAX_WIDTH."""
        want = int(self.fetch) if int(self.fetch) > 0 else 4 * int(limit)
        return max(min(want, MMR_MAX_WIDTH), min(int(limit), MMR_MAX_WIDTH))


def candidates(rel: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """bool per slot: the id is not -1, rel is finite and no earlier slot holds the same id."""
    seen, out = set(), np.zeros(ids.size, dtype=bool)
    for i, v in enumerate(ids.tolist()):
        out[i] = v != -1 and bool(np.isfinite(rel[i])) and v not in seen
        seen.add(v)
    return out


def mmr_host(rel, sim: Union[np.ndarray, Callable[[int, int], Sequence[float]]], lam: float, k: int,
             ids: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The MMR walk over one list of n slots (the slots below the count).
      rel  [n] relevance; ids [n] int64 (default: the slot numbers) -- ties go to the lower id
      sim  [n, n] pair cosines, NaN where a pair is not comparable, or a callable (slot of the pick, pick number t) -> that
           pick's row of n cosines (the kernel's d_out_sim_rows[t] replays a run)
    Returns (slots int64 [count], values float32 [count]) in pick order, count = min(k, candidates)."""
    rel = np.asarray(rel, dtype=np.float32).reshape(-1)
    n = rel.size
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size != n:
        raise ValueError("ids and rel must have one entry per slot")
    lam32 = np.float32(lam)
    if not np.float32(0.0) <= lam32 <= np.float32(1.0):
        raise ValueError(f"lam must be finite, in [0, 1] (got {lam})")
    mu32 = np.float32(1.0) - lam32
    cand = candidates(rel, ids)
    left = cand.copy()
    pen = np.zeros(n, dtype=np.float32)
    met = np.zeros(n, dtype=bool)
    slots, values = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(int(k)):
            if not left.any():
                break
            value = lam32 * rel - mu32 * pen          # fp32 mul, mul, sub: one rounding each
            live = np.flatnonzero(left)
            best = live[value[live] == value[live].max()]
            pick = int(best[np.argmin(ids[best])])
            slots.append(pick)
            values.append(value[pick])
            left[pick] = False
            row = np.asarray(sim(pick, t) if callable(sim) else sim[pick], dtype=np.float32).reshape(-1)
            hit = cand & ~np.isnan(row)
            pen[hit] = np.where(met[hit], np.maximum(pen[hit], row[hit]), row[hit])
            met |= hit
    return np.asarray(slots, dtype=np.int64), np.asarray(values, dtype=np.float32)
