"""The snippet-window rule of DESIGN.md 4.7e by brute force (include/crag_dense.h states it at crag_bm25_snippets_host).

Rows are token sequences (term ids).  For a pair the oracle tries EVERY start 0 .. the largest position that holds a
term of the query, not only the occurrences: score(s) is the numpy-fp32 sum, in slot order, of the weights of the slots
that have a position in [s, s + W).  It then checks the claim the kernel rests on -- a start moved right to the first
occurrence inside its window scores no less, so the largest score over all starts is reached at an occurrence -- and
answers with the lowest occurrence of the largest score."""
import numpy as np

WHERE_MAX = 65535     # positions at or above this are not indexed: they do not exist for the rule


def window_of(tokens, terms, weights, window):
    """One pair: tokens the row's term ids, terms / weights the query's slots.  -> (start, last, score fp32, covered)."""
    tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)[:WHERE_MAX]
    weights = np.asarray(weights, dtype=np.float32)
    holds = [tokens == t for t in terms]                      # per slot: where its term stands
    is_occ = np.zeros(tokens.size, dtype=bool)
    for h in holds:
        is_occ |= h
    if not is_occ.any():
        return -1, 0, np.float32(0.0), 0
    top = int(np.flatnonzero(is_occ)[-1])                     # the largest position that can matter
    starts = np.arange(top + 1)
    ends = np.minimum(starts + int(window), top + 1)
    sums = np.zeros(top + 1, dtype=np.float32)
    inside = []
    for j, h in enumerate(holds):
        before = np.concatenate([[0], np.cumsum(h[:top + 1])])  # occurrences of slot j below a position
        hit = before[ends] - before[starts] > 0
        inside.append(hit)
        sums = np.where(hit, sums + weights[j], sums)           # fp32 + fp32, slot after slot
    assert sums.dtype == np.float32
    # the claim: moving a start right to the first occurrence at or after it loses nothing (a window without an
    # occurrence scores +0.0, the least a sum of weights >= 0 can be)
    nxt = np.where(is_occ[:top + 1], starts, top + 1)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]
    assert np.all(sums[nxt] >= sums), "a start between occurrences beat the occurrence behind it"
    best = sums.max()
    assert best == sums[is_occ[:top + 1]].max()
    s = int(np.flatnonzero(is_occ[:top + 1] & (sums == best))[0])
    covered = sum(1 << j for j, hit in enumerate(inside) if hit[s])
    last = int(np.flatnonzero(is_occ[s:s + int(window)])[-1]) + s
    return s, last, sums[s], covered


def windows(rows, q_ptr, terms, weights, r_ptr, pair_rows, window):
    """The four outputs of crag_bm25_snippets_host for a batch: start int32, last int32, score fp32, covered uint64."""
    npairs = int(r_ptr[-1])
    start, last = np.empty(npairs, dtype=np.int32), np.empty(npairs, dtype=np.int32)
    score, covered = np.empty(npairs, dtype=np.float32), np.empty(npairs, dtype=np.uint64)
    for q in range(len(r_ptr) - 1):
        t0, t1 = int(q_ptr[q]), int(q_ptr[q + 1])
        for pair in range(int(r_ptr[q]), int(r_ptr[q + 1])):
            s, hi, sc, bits = window_of(rows[int(pair_rows[pair])], terms[t0:t1], weights[t0:t1], window)
            start[pair], last[pair], score[pair], covered[pair] = s, hi, sc, np.uint64(bits)
    return start, last, score, covered


def batch(queries, pairs):
    """queries: [(terms, weights)], pairs: per query the row positions -> q_ptr, terms, weights, r_ptr, rows."""
    q_ptr = np.zeros(len(queries) + 1, dtype=np.int32)
    np.cumsum([len(t) for t, _ in queries], out=q_ptr[1:])
    r_ptr = np.zeros(len(queries) + 1, dtype=np.int32)
    np.cumsum([len(p) for p in pairs], out=r_ptr[1:])
    terms = np.asarray([t for ts, _ in queries for t in ts], dtype=np.int32)
    weights = np.asarray([w for _, ws in queries for w in ws], dtype=np.float32)
    rows = np.asarray([r for p in pairs for r in p], dtype=np.int32)
    return q_ptr, terms, weights, r_ptr, rows


def random_case(seed=20261021, n_rows=200, row_len=300, n_terms=50, nq=8, q_terms=5):
    """The random case the host and the GPU tests share: rows, queries, every (query, row) pair."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, n_terms, size=row_len).tolist() for _ in range(n_rows)]
    queries = []
    for _ in range(nq):
        ts = np.sort(rng.choice(n_terms, size=q_terms, replace=False)).tolist()
        queries.append((ts, rng.uniform(0.5, 8.0, size=q_terms).astype(np.float32).tolist()))
    return rows, queries, [list(range(n_rows))] * nq
