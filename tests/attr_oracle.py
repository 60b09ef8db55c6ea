"""The rule of crag_attr_masks_host (include/crag_dense.h) in Python / numpy, in two forms:
`attr_masks_direct` reads the per-query clause lists as a request states them, one (query, row) pair at a time;
`attr_masks` reads the transposed (keys, key_sets, clause_sets) arrays the C entry takes and handles all rows at once
(what the tests use at tens of thousands of rows).  `transpose` turns the first form's input into the second's;
tests/test_attr_host.py holds the two against each other.  Both return a packed uint8 [nq, mask_stride] array."""
import numpy as np

MAX_CLAUSES = 8


def in_bit(in_mask, in_stride, q, i):
    """Bit (q, i) of an input mask: None admits every row; in_stride == 0 is one run shared by all queries."""
    if in_mask is None:
        return True
    run = np.asarray(in_mask, dtype=np.uint8).reshape(-1)
    return bool((run[(q * in_stride if in_stride else 0) + (i >> 3)] >> (i & 7)) & 1)


def attr_masks_direct(attr_ptr, attr_ids, n_attrs, queries, mask_stride, in_mask=None, in_stride=0):
    """queries: per query a list of clauses, each a list of key ids.  A row passes iff every clause holds a valid id
    (in [0, n_attrs)) that is among the row's ids."""
    n = len(attr_ptr) - 1
    out = np.zeros((len(queries), mask_stride), dtype=np.uint8)
    rows = [{int(a) for a in attr_ids[attr_ptr[i]:attr_ptr[i + 1]] if 0 <= int(a) < n_attrs} for i in range(n)]
    for q, clauses in enumerate(queries):
        for i in range(n):
            if in_bit(in_mask, in_stride, q, i) and all(rows[i].intersection(clause) for clause in clauses):
                out[q, i >> 3] |= 1 << (i & 7)
    return out


def transpose(queries):
    """(keys int32 ascending, key_sets uint64 [n_keys, 8], clause_sets uint64 [8]) of per-query clause lists."""
    clause_sets = [0] * MAX_CLAUSES
    sets = {}
    for q, clauses in enumerate(queries):
        assert len(clauses) <= MAX_CLAUSES
        for c, clause in enumerate(clauses):
            clause_sets[c] |= 1 << q
            for key in clause:
                sets.setdefault(int(key), [0] * MAX_CLAUSES)[c] |= 1 << q
    keys = np.asarray(sorted(sets), dtype=np.int32)
    key_sets = np.asarray([sets[int(k)] for k in keys], dtype=np.uint64).reshape(-1, MAX_CLAUSES)
    return keys, key_sets, np.asarray(clause_sets, dtype=np.uint64)


def attr_masks(attr_ptr, attr_ids, n_attrs, keys, key_sets, clause_sets, nq, mask_stride, in_mask=None, in_stride=0):
    """uint8 [nq, mask_stride]: bit (i & 7) of byte [q, i >> 3] is set iff i < n_rows, in(q, i) and for every c with
    bit q of clause_sets[c] some id a of row i, 0 <= a < n_attrs, equals keys[j] with bit q of key_sets[j][c]."""
    ptr = np.asarray(attr_ptr, dtype=np.int64)
    n = ptr.size - 1
    ids = np.asarray(attr_ids, dtype=np.int64)[:ptr[-1]] if n else np.empty(0, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.int64)
    key_sets = np.asarray(key_sets, dtype=np.uint64).reshape(-1, MAX_CLAUSES)
    have = np.zeros((n, MAX_CLAUSES), dtype=np.uint64)
    if ids.size and keys.size:
        row_of = np.repeat(np.arange(n), np.diff(ptr))
        at = np.minimum(np.searchsorted(keys, ids), keys.size - 1)
        hit = (keys[at] == ids) & (ids >= 0) & (ids < n_attrs)
        np.bitwise_or.at(have, row_of[hit], key_sets[at[hit]])
    passing = np.full(n, ~np.uint64(0), dtype=np.uint64)
    for c in range(MAX_CLAUSES):
        passing &= have[:, c] | ~np.uint64(clause_sets[c])
    out = np.zeros((nq, mask_stride), dtype=np.uint8)
    for q in range(nq):
        ok = (passing >> np.uint64(q)) & np.uint64(1) == 1
        bits = np.packbits(ok, bitorder="little")
        if in_mask is not None:
            run = np.asarray(in_mask, dtype=np.uint8).reshape(-1)[(q * in_stride if in_stride else 0):]
            bits &= run[:bits.size]
        out[q, :bits.size] = bits
    return out
