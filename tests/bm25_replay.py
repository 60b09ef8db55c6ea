"""fp32 replay of the BM25 lane: the formula of include/crag_dense.h (crag_bm25_lane_host) restated in numpy with every
intermediate an np.float32 -- one rounding per operation, in the header's order -- so that the device's result can be
compared bit for bit.  Written from the header, not from the kernel: no ranges, no rounds, no partial lists.

    x = float32(dl) / float32(avgdl);  x = x * 0.75f;  x = x + 0.25f;  x = x * 1.2f
    den = float32(tf) + x;  frac = float32(tf) / den;  acc = acc + w * frac        (terms in ascending term id)

A row is a candidate when its accumulator's bits are non-zero (a term touched it: every weight is positive) and its mask
bit is set.  Order: score bits descending (positive floats order as their bits), then row position ascending (ids ascend
with the position).  Padding: -1 for ids, NaN (0x7fc00000) for scores.  tests/bm25_oracle.py (fp64) stays the check of
the formula itself; tests/test_bm25_replay_host.py holds this file to it."""
import numpy as np

F32 = np.float32
NAN_BITS = np.uint32(0x7FC00000)


def accumulate(post_ptr, post_pos, post_tf, doc_len, avgdl, term_ids, weights):
    """fp32 accumulators [N] of one query (0.0 where no term of the query has a posting)."""
    doc_len = np.asarray(doc_len)
    acc = np.zeros(doc_len.size, dtype=F32)
    avg = F32(avgdl)
    term_ids, weights = np.asarray(term_ids), np.asarray(weights, dtype=F32)
    for i in np.argsort(term_ids, kind="stable"):
        a, b = int(post_ptr[term_ids[i]]), int(post_ptr[term_ids[i] + 1])
        pos = post_pos[a:b]                       # distinct inside a term
        tf = post_tf[a:b].astype(F32)
        x = doc_len[pos].astype(F32) / avg
        x = x * F32(0.75)
        x = x + F32(0.25)
        x = x * F32(1.2)
        den = tf + x
        frac = tf / den
        acc[pos] = acc[pos] + weights[i] * frac
    assert acc.dtype == F32
    return acc


def replay(post_ptr, post_pos, post_tf, doc_len, avgdl, term_ids, weights, k, ids, eligible=None):
    """One query -> (ids int64 [k], score bits uint32 [k], count).  ids None: ids are positions."""
    acc = accumulate(post_ptr, post_pos, post_tf, doc_len, avgdl, term_ids, weights)
    bits = acc.view(np.uint32)
    cand = bits != 0
    if eligible is not None:
        cand &= np.asarray(eligible, dtype=bool)
    pos = np.flatnonzero(cand)
    b = bits[pos].astype(np.int64)
    if pos.size > k:                               # only the rows at or above the k-th largest bits can be returned
        kth = np.partition(b, pos.size - k)[pos.size - k]
        keep = b >= kth
        pos, b = pos[keep], b[keep]
    order = np.lexsort((pos, -b))[:k]
    out_ids = np.full(k, -1, dtype=np.int64)
    out_bits = np.full(k, NAN_BITS, dtype=np.uint32)
    out_ids[:order.size] = pos[order] if ids is None else np.asarray(ids, dtype=np.int64)[pos[order]]
    out_bits[:order.size] = b[order].astype(np.uint32)
    return out_ids, out_bits, int(order.size)


def replay_index(index, q_ptr, term_ids, weights, k, eligible=None):
    """Every query of a batch over a Bm25Index -> (ids [nq, k], score bits [nq, k], counts [nq]).
    eligible: None, bool [N] (shared) or bool [nq, N]."""
    csr = getattr(index, "_replay_csr", None)
    if csr is None or csr[0] != len(index):        # (the index may have been extended)
        csr = index._replay_csr = (len(index),) + tuple(index.host_csr())
    nq = len(q_ptr) - 1
    out = np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), NAN_BITS, dtype=np.uint32), np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        el = None if eligible is None else (eligible[q] if np.ndim(eligible) == 2 else eligible)
        a, b = int(q_ptr[q]), int(q_ptr[q + 1])
        out[0][q], out[1][q], out[2][q] = replay(*csr[1:], index.doc_len, index.avgdl, term_ids[a:b], weights[a:b], k,
                                                 index.ids, el)
    return out


def assert_equals_replay(want, got_ids, got_scores, got_counts, what=""):
    """Exact: ids, counts, score bits and padding of a device result against replay_index's."""
    want_ids, want_bits, want_ct = want
    got_bits = np.ascontiguousarray(got_scores, dtype=np.float32).view(np.uint32)
    assert np.array_equal(got_counts, want_ct), f"{what}: counts {np.asarray(got_counts).tolist()} != {want_ct.tolist()}"
    for q in range(want_ids.shape[0]):
        bad = np.flatnonzero((got_ids[q] != want_ids[q]) | (got_bits[q] != want_bits[q]))
        assert bad.size == 0, (f"{what}: query {q}, first difference at rank {bad[0]}: id {got_ids[q][bad[0]]} bits "
                               f"{got_bits[q][bad[0]]:#010x}, replay id {want_ids[q][bad[0]]} bits "
                               f"{want_bits[q][bad[0]]:#010x} ({bad.size} ranks differ)")
