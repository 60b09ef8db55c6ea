"""crag_bm25_clause_masks_host on the GPU, through the C ABI on synthetic arrays, against tests/bm25_clause_oracle.py (the
rule of include/crag_dense.h restated over token sequences).  Every comparison is exact equality of the mask bytes over
the whole nq * mask_stride region of a buffer pre-filled with 0xA5, with a guard zone behind it that must stay 0xA5."""
import ctypes

import numpy as np
import pytest
import torch

from bm25_clause_oracle import (EXC_PHRASE, EXC_TERM, NOTHING, REQ_PHRASE, REQ_TERM, ClauseOracle, arrays_from_rows,
                                clauses_of, holds_phrase, packed, random_corpus, random_queries)
from cadence_rag_amd import _native
from cadence_rag_amd.bm25 import RANGE_ROWS as R
from cadence_rag_amd.bm25 import Bm25Index, parse_query
from cadence_rag_amd.dense_index import DenseIndex
from test_bm25_syntax_host import call_clause_masks, einval_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 4096
RT, XT, RP, XP = REQ_TERM, EXC_TERM, REQ_PHRASE, EXC_PHRASE


class Case:
    """Token sequences on the device (Bm25Index.from_arrays with planted positions) beside their oracle."""

    def __init__(self, rows, n_terms):
        self.n, self.n_terms = len(rows), n_terms
        row_ptr, terms, tfs, pair_off, pair_where = arrays_from_rows(rows)
        self.ix = Bm25Index.from_arrays(row_ptr, terms, tfs, n_terms, np.arange(self.n), DEV, pair_off=pair_off,
                                        pair_where=pair_where)
        self.oracle = ClauseOracle(rows)
        self.slot = _native.load().crag_upload_slot_create()
        assert self.slot

    def close(self):
        torch.cuda.synchronize()
        _native.load().crag_upload_slot_destroy(self.slot)
        self.ix.close()

    def run(self, queries, in_mask=None, extra=0, garbage=False, positions=True):
        """queries: [(kind, term ids)] per query.  in_mask: None, bool [N] or bool [nq, N]; garbage: set the input bits
        at or above n_rows.  Launches, checks the bytes and the guard, returns the oracle's bool [nq, N]."""
        nq = len(queries)
        stride = (self.n + 31) // 32 * 4 + extra
        c_ptr = np.zeros(nq + 1, dtype=np.int32)
        c_ptr[1:] = np.cumsum([len(c) for c in queries])
        flat = [c for cl in queries for c in cl]
        c_kind = np.asarray([k for k, _ in flat], dtype=np.int32)
        ct_ptr = np.zeros(len(flat) + 1, dtype=np.int32)
        ct_ptr[1:] = np.cumsum([len(t) for _, t in flat])
        ct_terms = np.asarray([t for _, ts in flat for t in ts], dtype=np.int32)
        d_in, in_stride = None, 0
        if in_mask is not None:
            pk = DenseIndex.pack_mask(in_mask)
            if garbage and self.n % 32:
                tail = np.zeros(pk.shape[-1] * 8, dtype=bool)
                tail[self.n:] = True
                pk = pk | np.packbits(tail, bitorder="little")
            d_in = torch.from_numpy(np.ascontiguousarray(pk)).to(DEV)
            in_stride = pk.shape[-1] if pk.ndim == 2 else 0
        out = torch.full((nq * stride + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        ix = self.ix
        rc = _native.load().crag_bm25_clause_masks_host(
            ix.d_post_ptr.data_ptr(), ix.d_post_pos.data_ptr(), ix.d_post_off.data_ptr() if positions else None,
            ix.d_post_where.data_ptr() if positions else None, self.n, self.n_terms, c_ptr.ctypes.data,
            c_kind.ctypes.data if c_kind.size else None, ct_ptr.ctypes.data, ct_terms.ctypes.data if ct_terms.size else None,
            nq, None if d_in is None else d_in.data_ptr(), in_stride, self.slot, out.data_ptr(), stride, None)
        assert rc == 0, _native.last_error()
        got = out.cpu().numpy()
        want_bool = self.oracle.mask(queries, in_mask)
        want = packed(want_bool, stride)
        assert np.all(got[nq * stride:] == 0xA5), "the guard zone behind the runs was written"
        bad = np.flatnonzero(got[:nq * stride] != want)
        assert bad.size == 0, (f"{bad.size} bytes differ, first: query {bad[0] // stride} byte {bad[0] % stride} "
                               f"got {got[bad[0]]:#04x} want {want[bad[0]]:#04x}")
        return want_bool


# ---- row counts, strides, input masks -------------------------------------------------------------------------------
def sparse_rows(n, seed):
    """Rows of 0-3 tokens over six terms; term 5 is rare."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, size=n)
    flat = rng.choice(6, size=int(lens.sum()), p=[0.3, 0.25, 0.2, 0.15, 0.09, 0.01])
    return np.split(flat, np.cumsum(lens)[:-1])


SPARSE_QUERIES = [[(RT, (0,))], [(XT, (1,))], [(RP, (0, 1))], [(XP, (1, 0))], [], [(RT, (2,)), (XT, (0,)), (XP, (2, 3))],
                  [(NOTHING, ())], [(RT, (5,))], [(RP, (0, 0)), (XT, (3,))]]


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("n", [1, 31, 32, 33, R - 1, R, R + 1, 2 * R + 5])
def test_row_counts_strides_and_input_masks(gpu, n, extra):
    rows = sparse_rows(n, 100 + n)
    if n == 1:
        rows = [np.array([0, 1])]
    case = Case(rows, 6)
    try:
        rng = np.random.default_rng(n)
        nq = len(SPARSE_QUERIES)
        case.run(SPARSE_QUERIES, None, extra)                                             # NULL: all ones below n_rows
        case.run(SPARSE_QUERIES, rng.random(n) < 0.7, extra, garbage=True)                # shared
        per_query = rng.random((nq, n)) < 0.7
        per_query[1] = True
        per_query[2] = False
        want = case.run(SPARSE_QUERIES, per_query, extra, garbage=True)
        assert np.array_equal(want[4], per_query[4]) and not want[2].any() and not want[6].any()   # no clause: a copy
        case.run(SPARSE_QUERIES[:1], None, extra)                                         # nq = 1
        case.run([[(RT, (0,))], [(XT, (1,))]], None, extra, positions=False)              # no phrase: no position arrays
    finally:
        case.close()


def test_batch_of_64_with_every_clause_count(gpu):
    """nq = 64: query q has q % 17 clauses (0 to 16, a query without clauses between queries with some)."""
    n = R + 77
    rng = np.random.default_rng(5)
    rows = [rng.choice(24, size=int(rng.integers(8, 20))) for _ in range(n)]
    case = Case(rows, 24)
    try:
        queries = []
        for q in range(64):
            row = rows[int(rng.integers(n))]
            cl = []
            for c in range(q % 17):
                kind = int(rng.integers(0, 4))
                if kind in (RT, XT):
                    cl.append((kind, (int(rng.integers(24)),)))
                else:
                    m = int(rng.integers(2, 4))
                    at = int(rng.integers(0, row.size - m + 1))
                    cl.append((kind, tuple(int(t) for t in (row[at:at + m] if kind == RP else rng.choice(24, size=m)))))
            queries.append(cl)
        assert [len(c) for c in queries[16:19]] == [16, 0, 1]
        want = case.run(queries, rng.random((64, n)) < 0.9, extra=8, garbage=True)
        assert want[17].sum() > 0.8 * n and want.any(axis=1).sum() > 8
    finally:
        case.close()


# ---- term clauses at the edges of ranges and words ------------------------------------------------------------------
def test_term_clauses_at_range_and_word_edges(gpu):
    n = 3 * R
    rng = np.random.default_rng(9)
    post = {
        0: [R, R + 160, R + 191, 2 * R - 1],                     # first / last position of a range and of a mask word
        1: np.concatenate([np.sort(rng.choice(R, 3000, replace=False)),           # absent from the middle range
                           2 * R + np.sort(rng.choice(R, 3000, replace=False))]),
        2: np.arange(R, 2 * R),                                  # covers the whole middle range
        3: [0, 31, 32, R - 1, R, 2 * R - 1, 2 * R, n - 1],
    }
    common = np.sort(rng.choice(n, 500, replace=False))
    for t in range(4, 20):                                       # sixteen terms that meet in `common`
        post[t] = np.union1d(common, rng.choice(n, 4000, replace=False))
    rows = [[] for _ in range(n)]
    for t in sorted(post):
        for p in np.asarray(post[t]).tolist():
            rows[p].append(t)
    case = Case(rows, 20)
    try:
        sixteen = [(RT, (t,)) for t in range(4, 20)]
        queries = [[(RT, (0,))], [(RT, (1,))], [(XT, (2,))], [(RT, (3,)), (XT, (3,))], sixteen, [(NOTHING, ())],
                   [(RT, (3,))], [(XT, (1,)), (XT, (2,))], [(RT, (4,)), (NOTHING, ()), (RT, (5,))],
                   sixteen[:15] + [(XT, (3,))]]
        want = case.run(queries)
        assert np.flatnonzero(want[0]).tolist() == post[0]
        assert want[1][:R].sum() == 3000 and not want[1][R:2 * R].any() and want[1][2 * R:].sum() == 3000
        assert want[2][:R].all() and not want[2][R:2 * R].any() and want[2][2 * R:].all()
        assert not want[3].any() and not want[5].any() and not want[8].any()
        assert set(common.tolist()) <= set(np.flatnonzero(want[4]).tolist()) and want[4].sum() < 600
        assert np.flatnonzero(want[6]).tolist() == post[3]
        case.run(queries, rng.random(n) < 0.5, extra=8)
    finally:
        case.close()


# ---- phrases ----------------------------------------------------------------------------------------------------------
A, B, C, D, X_, Z = 0, 1, 2, 3, 4, 5
EIGHT = tuple(range(6, 14))
PHRASE_ROWS = [
    [A, B, X_, X_],                                   # 0  "a b" at position 0
    [X_, X_, A, B],                                   # 1  ... at the row's last position
    [X_, A],                                          # 2  the last token of a row ...
    [B, X_],                                          # 3  ... and the first of the next: no match
    [A, B, A],                                        # 4
    [A, B, B, A],                                     # 5
    [A, A, B, A],                                     # 6
    [A] * 600,                                        # 7
    [X_, *EIGHT, X_],                                 # 8  the eight-term phrase
    [X_, *EIGHT[:6], EIGHT[7], EIGHT[6], X_],         # 9  ... its last two terms swapped
    [D] * 300 + [C] + [D] * 299,                      # 10 tf 1 against tf 599 in one row
    [A, X_, B],                                       # 11 both words, never adjacent
    [B, A],                                           # 12 ... in the other order
    [Z] * 65533 + [A, B],                             # 13 positions 65 533 and 65 534
    [Z] * 65534 + [A, B],                             # 14 position 65 535 is not indexed
    [C, D],                                           # 15
    [D] * 600,                                        # 16 no c
]


def test_phrases(gpu):
    case = Case(PHRASE_ROWS, 14)
    try:
        queries = [[(RP, (A, B))], [(XP, (A, B))], [(RP, (A, B, A))], [(RP, (A, A))], [(RP, EIGHT)], [(RP, (D, C, D))],
                   [(RP, (C, D))], [(RP, (D, C))], [(RP, (C, C))], [(XP, (A, A))], [(RP, (A, B)), (XP, (B, A))],
                   [(RP, (B, A)), (RT, (Z,))], [(RP, (D, D)), (XT, (C,))], [(RP, EIGHT[1:])], [(RP, (Z, A, B))]]
        want = case.run(queries)
        rows = lambda q: np.flatnonzero(want[q]).tolist()
        assert rows(0) == [0, 1, 4, 5, 6, 13] and rows(1) == [2, 3, 7, 8, 9, 10, 11, 12, 14, 15, 16]
        assert rows(2) == [4, 6] and rows(3) == [6, 7] and rows(4) == [8] and rows(5) == [10]
        assert rows(6) == [10, 15] and rows(7) == [10] and rows(8) == []
        assert rows(10) == [0, 1, 13] and rows(11) == [] and rows(12) == [16] and rows(13) == [8] and rows(14) == [13]
        case.run(queries, np.arange(len(PHRASE_ROWS)) % 3 != 1, extra=8, garbage=True)
        # an index without position arrays: the phrase is refused, nothing is written
        out = torch.full((64,), 0xA5, dtype=torch.uint8, device=DEV)
        ix = case.ix
        rc = _native.load().crag_bm25_clause_masks_host(
            ix.d_post_ptr.data_ptr(), ix.d_post_pos.data_ptr(), None, None, case.n, 14,
            np.array([0, 1], np.int32).ctypes.data, np.array([2], np.int32).ctypes.data,
            np.array([0, 2], np.int32).ctypes.data, np.array([A, B], np.int32).ctypes.data, 1, None, 0, case.slot,
            out.data_ptr(), 4, None)
        assert rc == -1 and np.all(out.cpu().numpy() == 0xA5)
    finally:
        case.close()


# ---- one seeded random corpus ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_case(gpu):
    rows = random_corpus()
    case = Case(rows, 50)
    yield case, rows
    case.close()


def test_random_corpus(random_case):
    case, rows = random_case
    texts = random_queries(rows)
    parsed = [parse_query(t) for t in texts]
    queries = [clauses_of(p, case.ix.vocab.get) for p in parsed]
    assert len(queries) == 64 and all(1 <= len(c) <= 3 for c in queries)
    assert {k for c in queries for k, _ in c} == {RT, XT, RP, XP}
    # on the oracle alone: every query passes at least one row and fewer than all rows
    alone = case.oracle.mask(queries)
    assert np.all(alone.sum(axis=1) >= 1) and np.all(alone.sum(axis=1) < case.n)
    # ... and at least 16 queries contain a phrase that some row holds as words but not adjacent
    apart = 0
    for cl in queries:
        hit = False
        for kind, terms in cl:
            if kind in (RP, XP):
                words = np.ones(case.n, dtype=bool)
                for t in set(terms):
                    words &= case.oracle.holds_term(t)
                hit |= bool((words & ~case.oracle.holds_phrase_rows(terms)).any())
        apart += hit
    assert apart >= 16, apart
    rng = np.random.default_rng(3)
    case.run(queries)
    case.run(queries, rng.random(case.n) < 0.5, extra=8)
    case.run(queries, rng.random((64, case.n)) < 0.5, garbage=True)
    r = 12345                                          # the vectorised oracle against the one-row definition
    for cl in queries[:8]:
        for kind, terms in cl:
            if kind in (RP, XP):
                assert case.oracle.holds_phrase_rows(terms)[r] == holds_phrase(rows[r], terms)


# ---- the frame the clause kernel shares with the any-of groups ----------------------------------------------------------
def test_term_clauses_are_any_of_groups_of_one_term(gpu):
    """REQ_TERM t == REQ_ANY {t}, EXC_TERM t == EXC_ANY {t}, MATCH_NOTHING == REQ_ANY {}: the same bytes from
    crag_bm25_clause_masks_host and crag_bm25_group_masks_host, and the oracle's.  n = RANGE + 1 (the second range holds
    one row), 8 bytes of stride padding, a per-query input mask with its last valid bit set and row RANGE - 1 cleared;
    term 0 is held by every row, term 1 by rows RANGE - 1 and RANGE alone, term 2 by none."""
    n = R + 1
    rows = [np.array([0])] * (R - 1) + [np.array([0, 1])] * 2
    case = Case(rows, 3)
    try:
        ix, lib = case.ix, _native.load()
        stride = (n + 31) // 32 * 4 + 8
        in_mask = np.ones((3, n), dtype=bool)
        in_mask[:, R - 1] = False
        in_mask[1, 7] = in_mask[2, R - 2] = False                       # (per query: the runs differ)
        d_in = torch.from_numpy(np.ascontiguousarray(DenseIndex.pack_mask(in_mask))).to(DEV)
        in_stride = d_in.shape[-1]
        ptr, t_ptr1, t_ptr0 = np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
        terms = np.arange(3, dtype=np.int32)

        def launch(entry, extra, kind, t_ptr):
            kinds = np.full(3, kind, dtype=np.int32)
            out = torch.full((3 * stride + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
            rc = getattr(lib, entry)(ix.d_post_ptr.data_ptr(), ix.d_post_pos.data_ptr(), *extra, n, 3, ptr.ctypes.data,
                                     kinds.ctypes.data, t_ptr.ctypes.data, terms.ctypes.data if t_ptr[-1] else None, 3,
                                     d_in.data_ptr(), in_stride, case.slot, out.data_ptr(), stride, None)
            assert rc == 0, _native.last_error()
            got = out.cpu().numpy()
            assert np.all(got[3 * stride:] == 0xA5), "the guard zone behind the runs was written"
            return got[:3 * stride]

        where = (ix.d_post_off.data_ptr(), ix.d_post_where.data_ptr())
        for clause_kind, group_kind, t_ptr in [(RT, 0, t_ptr1), (XT, 1, t_ptr1), (NOTHING, 0, t_ptr0)]:
            queries = [[(clause_kind, (t,) if t_ptr[-1] else ())] for t in range(3)]
            want = packed(case.oracle.mask(queries, in_mask), stride)
            by_clause = launch("crag_bm25_clause_masks_host", where, clause_kind, t_ptr)
            by_group = launch("crag_bm25_group_masks_host", (), group_kind, t_ptr)
            assert np.array_equal(by_clause, by_group) and np.array_equal(by_clause, want), (clause_kind, group_kind)
            for got in (by_clause, by_group):                           # the stride padding is zero
                assert not got.reshape(3, stride)[:, (n + 31) // 32 * 4:].any()
        # what the shapes are for: the required rare term keeps row RANGE alone, the last valid bit of the second range
        rare = case.oracle.mask([[(RT, (1,))]], in_mask[:1])[0]
        assert rare[R] and rare.sum() == 1
    finally:
        case.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_every_einval_leaves_the_buffer_untouched(gpu):
    rng = np.random.default_rng(11)
    rows = [rng.choice(7, size=6) for _ in range(100)]
    rows[5] = np.array([0, 1, 2, 3, 4, 5, 6])
    case = Case(rows, 7)
    try:
        ix = case.ix
        out = torch.full((16 + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        base = dict(post_ptr=ix.d_post_ptr.data_ptr(), post_pos=ix.d_post_pos.data_ptr(), post_off=ix.d_post_off.data_ptr(),
                    post_where=ix.d_post_where.data_ptr(), slot=case.slot, out=out.data_ptr())
        lib = _native.load()
        for bad in einval_cases(out.data_ptr()):
            assert call_clause_masks(lib, 0, **{**base, **bad}) == -1, bad
            assert b"bm25_clause_masks_host" in lib.crag_last_error(), bad
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == 0xA5)
        # the call the cases vary is itself valid: +0 "1 2" over 100 rows
        assert call_clause_masks(lib, 0, **base) == 0, _native.last_error()
        want = packed(case.oracle.mask([[(RT, (0,)), (RP, (1, 2))]]), 16)
        got = out.cpu().numpy()
        assert np.array_equal(got[:16], want) and np.all(got[16:] == 0xA5) and want[0] & 0x20    # row 5 passes
        # n_rows == 0 is CRAG_OK: the runs are zeroed
        out.fill_(0xA5)
        assert call_clause_masks(lib, 0, **{**base, "n": 0, "stride": 8}) == 0, _native.last_error()
        got = out.cpu().numpy()
        assert np.all(got[:8] == 0) and np.all(got[8:] == 0xA5)
    finally:
        case.close()
