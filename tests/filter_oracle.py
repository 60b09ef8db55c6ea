"""The rule of crag_filter_masks_host (include/crag_dense.h) in numpy: `filter_bit` is the rule for one (query, row)
pair as the header states it; `filter_masks` applies the same three clauses to all rows of a query at once (what the
tests use at tens of thousands of rows; tests/test_filter_host.py holds the two against each other)."""
import numpy as np

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max


def filter_bit(ts, slot, n_calls, qset, lo, hi, q):
    ok = qset is None or (0 <= slot < n_calls and (int(qset[slot]) >> q) & 1 == 1)
    ok = ok and (lo == I64_MIN or (ts != I64_MIN and ts >= lo))
    return ok and (hi == I64_MAX or (ts != I64_MIN and ts <= hi))


def filter_masks(started_us, call_slot, n_calls, qset, date_from, date_to, mask_stride):
    """uint8 [nq, mask_stride]: bit (i & 7) of byte [q, i >> 3] is set iff row i passes query q; every other bit is 0."""
    ts, slot = np.asarray(started_us, dtype=np.int64), np.asarray(call_slot, dtype=np.int64)
    out = np.zeros((len(date_from), mask_stride), dtype=np.uint8)
    known = (slot >= 0) & (slot < n_calls)
    for q in range(len(date_from)):
        ok = np.ones(ts.size, dtype=bool)
        if qset is not None:
            ok = known.copy()
            ok[known] = (np.asarray(qset, dtype=np.uint64)[slot[known]] >> np.uint64(q)) & np.uint64(1) == 1
        if int(date_from[q]) != I64_MIN:
            ok &= (ts != I64_MIN) & (ts >= int(date_from[q]))
        if int(date_to[q]) != I64_MAX:
            ok &= (ts != I64_MIN) & (ts <= int(date_to[q]))
        bits = np.packbits(ok, bitorder="little")
        out[q, :bits.size] = bits
    return out
