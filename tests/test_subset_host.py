"""The listed-rows search, host side (no GPU): DenseTable.scoped_positions equals np.flatnonzero(filter_mask(...)) for
every call-scoped request without a pass over all rows, says None where the route does not apply, and follows the
table's generation; the C entries exist, size their scratch sensibly and refuse bad arguments before touching a device."""
from datetime import datetime, timedelta
from uuid import UUID

import numpy as np
import pytest

from cadence_rag_amd import _native
from cadence_rag_amd import retrieve as rt
from tests.test_filter_host import make_table, some_timestamp

F = rt.RetrieveFilters


def table_of(seed, n, n_calls):
    table, calls = make_table(np.random.default_rng(seed), n, n_calls=n_calls)
    table.generation = 1
    return table, calls


def scoped_cases(table, calls):
    at = some_timestamp(table)
    some = calls[: max(2, len(calls) // 3)]
    return [
        (F(), calls[:1]),
        (F(), some),
        (F(), list(calls)),
        (F(), some + some[:1]),                                  # a call id given twice
        (F(date_from=at), some),
        (F(date_to=at), some),
        (F(date_from=at - timedelta(hours=30), date_to=at), some),
        (F(date_from=at + timedelta(days=400)), some),           # nothing passes
        (F(call_tags=["outage"]), list(calls)),
        (F(call_tags=["billing", "renewal"]), some),
        (F(call_tags=["no-such-tag"]), some),
        (F(call_tags=["billing"], date_from=at - timedelta(hours=50)), calls[1:]),
        (F(), calls[-1:] + [UUID(int=7)]),                       # an id no row has
        (F(), [UUID(int=7)]),
        (F(), []),                                               # an empty list admits nothing
        (F(date_to=at, call_tags=["onboarding"]), []),
    ]


@pytest.mark.parametrize("n, n_calls", [(1, 1), (33, 4), (200, 20), (500, 23)])
def test_scoped_positions_equal_the_mask(n, n_calls):
    table, calls = table_of(10 + n, n, n_calls)
    assert np.isnat(table.call_started_at).any() or n == 1
    for filters, call_ids in scoped_cases(table, calls):
        want = np.flatnonzero(table.filter_mask(filters, call_ids))
        got = table.scoped_positions(filters, call_ids, n)
        assert got is not None and got.dtype.kind == "i" and got.ndim == 1, (filters, call_ids)
        assert np.array_equal(got, want), (filters, call_ids)


def test_all_nat_rows():
    table, calls = make_table(np.random.default_rng(3), 70, n_calls=5, nat_share=1.0)
    table.generation = 1
    at = datetime(2024, 5, 2)
    for filters in (F(), F(date_from=at), F(date_to=at), F(date_from=at - timedelta(days=9), date_to=at)):
        want = np.flatnonzero(table.filter_mask(filters, calls[:3]))
        assert np.array_equal(table.scoped_positions(filters, calls[:3], 70), want)
        assert (want.size > 0) == (not (filters.date_from or filters.date_to))


def test_where_the_route_does_not_apply():
    table, calls = table_of(5, 120, 9)
    assert table.scoped_positions(None, calls[:2], 1000) is None        # filters=None: call ids are not honoured
    assert table.filter_mask(None, calls[:2]) is None
    assert table.scoped_positions(F(), None, 1000) is None
    assert table.scoped_positions(F(call_tags=["outage"]), None, 1000) is None
    assert table.scoped_positions(None, None, 1000) is None
    # the limit counts the rows of the scoped calls, before dates and tags
    scoped = int(np.count_nonzero(table.filter_mask(F(), calls[:3])))
    assert scoped > 1
    at = some_timestamp(table)
    for filters in (F(), F(date_from=at), F(call_tags=["outage"])):
        assert table.scoped_positions(filters, calls[:3], scoped - 1) is None
        got = table.scoped_positions(filters, calls[:3], scoped)
        assert np.array_equal(got, np.flatnonzero(table.filter_mask(filters, calls[:3])))
    assert table.scoped_positions(F(), calls[:3], 0) is None
    assert table.scoped_positions(F(), [], 0).size == 0


def test_the_map_follows_the_generation():
    table, calls = table_of(6, 90, 6)
    before = table.scoped_positions(F(), calls[:2], 90)
    first_map = table._call_positions()
    assert table._call_positions() is first_map                          # built once per (generation, length)
    # the columns change together with the generation: rows are dropped and the calls reassigned
    keep = np.ones(90, dtype=bool)
    keep[before[::2]] = False
    table.call_ids = table.call_ids[keep][::-1].copy()
    table.call_started_at = table.call_started_at[keep][::-1].copy()
    table.index.n = int(keep.sum())
    table.generation += 1
    after = table.scoped_positions(F(), calls[:2], 90)
    assert table._call_positions() is not first_map
    assert np.array_equal(after, np.flatnonzero(table.filter_mask(F(), calls[:2])))
    assert not np.array_equal(after, before)


def test_binding_and_header_agree():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "crag_dense.h").read_text()
    assert int(re.search(r"#define CRAG_SUBSET_MAX_WIDTH (\d+)", text).group(1)) == _native.CRAG_SUBSET_MAX_WIDTH == 4096
    assert "crag_index_search_ids_async" in _native.SIGNATURES and "crag_index_search_ids_scratch_bytes" in _native.SIGNATURES


def test_scratch_bytes(native_lib):
    fn = native_lib.crag_index_search_ids_scratch_bytes
    sizes = {(nq, w): int(fn(nq, w)) for nq in (1, 2, 33, 70) for w in (1, 63, 64, 65, 200, 4096)}
    assert all(v > 0 and v % 8 == 0 for v in sizes.values())
    for (nq, w), v in sizes.items():
        assert all(v < sizes[(nq2, w)] for nq2 in (1, 2, 33, 70) if nq2 > nq)
        assert all(v < sizes[(nq, w2)] for w2 in (1, 63, 64, 65, 200, 4096) if w2 > w)
        assert v >= nq * w * 8                                             # a 64-bit key per slot


def test_argument_errors_are_codes_with_a_message(native_lib):
    """Checked before any HIP call: stand-in pointers are never dereferenced."""
    fn = native_lib.crag_index_search_ids_async
    some = np.zeros(64, dtype=np.uint64)
    P = some.ctypes.data

    def call(ix=P, queries=P, nq=2, ids=P, counts=P, width=8, stride=None, k=5, out_ids=P, out_scores=P, out_counts=P,
             slot=None, scratch=P, scratch_bytes=1 << 20):
        return fn(ix, queries, nq, ids, counts, width, width if stride is None else stride, k, out_ids, out_scores,
                  out_counts, slot, scratch, scratch_bytes, None)

    bad = [dict(ix=None), dict(queries=None), dict(ids=None), dict(counts=None), dict(out_ids=None), dict(out_scores=None),
           dict(out_counts=None), dict(scratch=None), dict(nq=-1), dict(width=0), dict(width=-5), dict(k=0), dict(k=129),
           dict(stride=4), dict(stride=16), dict(stride=-8), dict(scratch_bytes=2 * 8 * 8 - 1), dict(scratch_bytes=0),
           dict(scratch=P + 4)]
    for kw in bad:
        assert call(**kw) == -1, kw                # CRAG_EINVAL
        assert b"search_ids" in native_lib.crag_last_error(), kw
    assert call(width=4097) == -5                  # CRAG_E2BIG: the caller uses the mask route
    assert b"4096" in native_lib.crag_last_error()
    assert call(nq=0) == 0                         # nothing to do
