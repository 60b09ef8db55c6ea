"""Plain Python / numpy statement of the three contracts behind a hybrid /retrieve answer -- reciprocal-rank fusion,
the exact-token lane and the cross-shard result merge -- written from the documented semantics
(include/crag_dense.h, cadence_rag_amd.retrieve._rrf_merge), not from the kernels.  No torch, no GPU.

The only thing shared with the code under test are the two multiplicative-hash constants of the kernels' LDS tables
(colliding_fuse_ids / colliding_tech_hashes), which the tests need to aim keys at a chosen table slot."""
from __future__ import annotations

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
FUSE_SLOTS = 2048
TECH_SLOTS = 4096


# ------------------------------------------------------------------------------------------------
# reciprocal-rank fusion
# ------------------------------------------------------------------------------------------------
def rrf(lanes_ids, lanes_counts, widths, rrf_k, out_k):
    """lanes_ids[l]: [nq, widths[l]] int64, lanes_counts[l]: [nq] ints.  Per query: clamp each count to [0, width];
    walk the lanes in lane order and each lane in rank order (rank from 1) and add 1.0 / (rrf_k + rank) to the key's
    score in Python floats -- a key repeated inside a lane adds again, exactly as _rrf_merge does --; bit l of the
    key's mask = lane l returned it; stable sort by score descending (ties keep first-insertion order); cut at out_k.
    Returns ids [nq, out_k] int64 (-1 pad), scores [nq, out_k] float64 (NaN pad), masks [nq, out_k] uint32 (0 pad),
    counts [nq] int32 = min(unique keys, out_k)."""
    nq = int(np.asarray(lanes_counts[0]).shape[0])
    ids = np.full((nq, out_k), -1, dtype=np.int64)
    scores = np.full((nq, out_k), np.nan, dtype=np.float64)
    masks = np.zeros((nq, out_k), dtype=np.uint32)
    counts = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        score, mask = {}, {}                       # dicts keep insertion order
        for l, (lane, cnt, width) in enumerate(zip(lanes_ids, lanes_counts, widths)):
            c = min(max(int(cnt[q]), 0), int(width))
            for rank in range(1, c + 1):
                key = int(lane[q][rank - 1])
                score[key] = score.get(key, 0.0) + 1.0 / (rrf_k + rank)
                mask[key] = mask.get(key, 0) | (1 << l)
        order = sorted(score.items(), key=lambda kv: kv[1], reverse=True)[:out_k]   # sorted() is stable
        counts[q] = len(order)
        for j, (key, s) in enumerate(order):
            ids[q, j], scores[q, j], masks[q, j] = key, s, mask[key]
    return ids, scores, masks, counts


# ------------------------------------------------------------------------------------------------
# exact-token lane
# ------------------------------------------------------------------------------------------------
def _fold(h):
    h = np.asarray(h, dtype=np.uint64).copy()
    h[h == 0] = 1                                  # hashes 0 and 1 are one token to the lane
    return h


def tech_lane(order, row_ptr, tokens, ids, qtok, qtok_n, k, mask=None, mask_stride=0):
    """order [n] int32: table position of the row at rank r; row_ptr [n+1] / tokens [nnz] uint64: the rows' token hashes
    in CSR form BY RANK; ids [n] by table position, or None (the position itself); qtok [nq, 32] uint64 of which the
    first qtok_n[q] count; mask: packed bits per table POSITION as uint8 (bit p & 7 of byte q * mask_stride + (p >> 3);
    mask_stride 0 = one mask for all queries).  A rank matches a query when its token set meets the query's tokens and
    the mask (if any) admits its position; the answer is the first k matching ranks, as ids.
    Returns ids [nq, k] int64 (-1 pad), counts [nq] int32."""
    order = np.asarray(order, dtype=np.int64)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = order.shape[0]
    nnz = int(row_ptr[n])
    toks = _fold(np.asarray(tokens, dtype=np.uint64)[:nnz])
    rank_of_tok = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    qtok = np.asarray(qtok, dtype=np.uint64)
    nq = qtok.shape[0]
    out = np.full((nq, k), -1, dtype=np.int64)
    counts = np.zeros(nq, dtype=np.int32)
    mask = None if mask is None else np.asarray(mask, dtype=np.uint8).reshape(-1)
    for q in range(nq):
        mine = _fold(qtok[q, :max(int(qtok_n[q]), 0)])
        if n == 0 or mine.size == 0:
            continue
        hit = np.isin(toks, mine)
        match = np.bincount(rank_of_tok[hit], minlength=n) > 0
        if mask is not None:
            byte = mask[q * int(mask_stride) + (order >> 3)]
            match &= ((byte >> (order & 7).astype(np.uint8)) & 1).astype(bool)
        ranks = np.flatnonzero(match)[:k]
        pos = order[ranks]
        out[q, :ranks.size] = pos if ids is None else np.asarray(ids, dtype=np.int64)[pos]
        counts[q] = ranks.size
    return out, counts


# ------------------------------------------------------------------------------------------------
# cross-shard merge
# ------------------------------------------------------------------------------------------------
def ordered_bits(scores):
    """fp32 -> uint32 whose unsigned order is the total order of the floats' bit patterns: negative values below
    positive ones, -0.0 directly below +0.0."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def merge(ids, scores, counts, k):
    """ids / scores [n_lists, nq, k] int64 / fp32, counts [n_lists, nq]: the first counts[l, q] entries of every list
    are candidates.  Order: the fp32 score's ORDERED BIT PATTERN descending, then id ascending; the first k.
    This is tests/helpers.cpu_merge_topk except for signed zeros: there -0.0 == +0.0 and the id decides, here -0.0
    sorts below +0.0 whatever the ids (the library's rule: it ranks the bit patterns).
    Returns ids [nq, k] (-1 pad), scores [nq, k] fp32 (NaN pad), counts [nq] int32."""
    ids = np.asarray(ids, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    n_lists, nq, kk = ids.shape
    assert kk == k
    out_ids = np.full((nq, k), -1, dtype=np.int64)
    out_sc = np.full((nq, k), np.nan, dtype=np.float32)
    out_ct = np.zeros(nq, dtype=np.int32)
    ob = ordered_bits(scores)
    for q in range(nq):
        cand = []
        for l in range(n_lists):
            for j in range(min(max(int(counts[l][q]), 0), k)):
                cand.append((-int(ob[l, q, j]), int(ids[l, q, j]), l, j))
        cand.sort()
        cand = cand[:k]
        out_ct[q] = len(cand)
        for r, (_, i, l, j) in enumerate(cand):
            out_ids[q, r] = i
            out_sc[q, r] = scores[l, q, j]
    return out_ids, out_sc, out_ct


# ------------------------------------------------------------------------------------------------
# keys aimed at one slot of the kernels' open-addressing tables
# ------------------------------------------------------------------------------------------------
def fuse_slot(ids):
    """Home slot of an id in the fusion kernel's 2048-slot key table."""
    x = np.asarray(ids, dtype=np.int64).view(np.uint64) * _GOLDEN          # wraps mod 2^64
    return ((x >> np.uint64(40)) & np.uint64(FUSE_SLOTS - 1)).astype(np.int64)


def tech_slot(hashes):
    """Home slot of a (folded) token hash in the token lane's 4096-slot table: the top 12 bits of the product."""
    x = np.asarray(hashes, dtype=np.uint64) * _GOLDEN
    return (x >> np.uint64(52)).astype(np.int64)


def _search(slot_of, start, slot, n, dtype):
    found, have, base, step = [], 0, int(start), 1 << 20
    while have < n:
        cand = np.arange(base, base + step, dtype=np.uint64).astype(dtype)
        hit = cand[slot_of(cand) == slot]
        found.append(hit)
        have += hit.size
        base += step
    return np.concatenate(found)[:n]


def colliding_fuse_ids(slot, n):
    """n distinct int64 ids >= 0 whose home slot in the fusion table is `slot` (1 candidate in 2048 hits)."""
    return _search(fuse_slot, 1, slot, n, np.int64)


def colliding_tech_hashes(slot, n):
    """n distinct uint64 hashes >= 2 whose home slot in the token table is `slot` (1 candidate in 4096 hits)."""
    return _search(tech_slot, 2, slot, n, np.uint64)
