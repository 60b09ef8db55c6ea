"""numpy oracle of the grouped search (crag_index_search_grouped_async), one query at a time, in the two
forms the contract states: the walk over the ranking, and the top-k of the union of every group's own top-g.  Scores are
ranked the way the lane's 64-bit keys rank them -- by the orderable bits of the fp32 score (+0 above -0), then by
ascending id -- so an oracle result can be compared bit for bit."""
from __future__ import annotations

import numpy as np


def orderable(scores) -> np.ndarray:
    """fp32 -> uint32 whose unsigned order is the order of the floats (f2ord of csrc/crag_exact.h)."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _rows_that_count(groups, eligible, n_groups):
    groups = np.asarray(groups, dtype=np.int64)
    ok = np.asarray(eligible, dtype=bool) & (groups >= 0)
    if n_groups is not None:
        ok &= groups < int(n_groups)
    return groups, ok


def _ranked(scores, ids, ok) -> np.ndarray:
    """positions of the rows that count, best first: score descending, then id ascending"""
    pos = np.flatnonzero(ok)
    key = orderable(np.asarray(scores, dtype=np.float32)[pos]).astype(np.int64)
    return pos[np.lexsort((np.asarray(ids, dtype=np.int64)[pos], -key))]


def _padded(scores, ids, groups, chosen, k):
    out_ids = np.full(k, -1, dtype=np.int64)
    out_scores = np.full(k, np.nan, dtype=np.float32)
    out_groups = np.full(k, -1, dtype=np.int32)
    n = len(chosen)
    if n:
        chosen = np.asarray(chosen, dtype=np.int64)
        out_ids[:n] = np.asarray(ids, dtype=np.int64)[chosen]
        out_scores[:n] = np.asarray(scores, dtype=np.float32)[chosen]
        out_groups[:n] = groups[chosen]
    return out_ids, out_scores, out_groups, n


def capped_topk(scores, ids, groups, eligible, k, g, n_groups=None):
    """The walk: rank the eligible rows, keep a row iff its group holds fewer than g kept rows, stop at k.  A row whose
    group number is negative (or >= n_groups when given) is ignored.  -> (ids [k] -1 pad, scores [k] NaN pad, groups [k]
    -1 pad, count)."""
    groups, ok = _rows_that_count(groups, eligible, n_groups)
    kept, held = [], {}
    for p in _ranked(scores, ids, ok):
        if len(kept) == k:
            break
        grp = int(groups[p])
        if held.get(grp, 0) < g:
            held[grp] = held.get(grp, 0) + 1
            kept.append(int(p))
    return _padded(scores, ids, groups, kept, k)


def union_topk(scores, ids, groups, eligible, k, g, n_groups=None):
    """The same result as the top-k of the union of every group's own top-g."""
    groups, ok = _rows_that_count(groups, eligible, n_groups)
    union = np.zeros(len(groups), dtype=bool)
    for grp in np.unique(groups[ok]):
        union[_ranked(scores, ids, ok & (groups == grp))[:g]] = True
    return _padded(scores, ids, groups, _ranked(scores, ids, union)[:k].tolist(), k)
