"""Filter masks, host side (no GPU): compile_predicates + the numpy rule of the kernel (tests/filter_oracle.py) equal
pack_mask(DenseTable.filter_mask(...)) bit for bit, quirks included, and the C entry refuses bad arguments with a code
and a message before it touches the device."""
from datetime import datetime, timedelta, timezone
from uuid import UUID

import numpy as np
import pytest

from cadence_rag_amd import filters as fl
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.dense_index import DenseIndex
from tests import filter_oracle

T0 = datetime(2024, 5, 1, 12, 0, 0)
TAGS = ("billing", "outage", "onboarding", "renewal")


class _Rows:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def make_table(rng, n, n_calls=None, nat_share=0.2):
    """A DenseTable without an index: filter_mask reads the host columns and len() only."""
    n_calls = n_calls or max(1, min(n, int(rng.integers(1, 12))))
    calls = [UUID(int=100 + c) for c in range(n_calls)]
    table = object.__new__(rt.DenseTable)
    table.index = _Rows(n)
    table.call_ids = np.asarray([calls[int(c)] for c in rng.integers(0, n_calls, n)], dtype=object)
    started = np.asarray([np.datetime64(T0 + timedelta(hours=int(h)), "us") for h in rng.integers(0, 240, n)],
                         dtype="datetime64[us]")
    started[rng.random(n) < nat_share] = np.datetime64("NaT")
    table.call_started_at = started
    # every third call is missing from call_tags, one has None, the others one or two tags
    table.call_tags = {c: (None if i % 7 == 4 else [TAGS[i % 4]] + ([TAGS[(i + 1) % 4]] if i % 2 else []))
                       for i, c in enumerate(calls) if i % 3 != 2}
    return table, calls


def some_timestamp(table):
    real = table.call_started_at[~np.isnat(table.call_started_at)]
    return real[len(real) // 2].astype(datetime) if real.size else T0


def cases(table, calls):
    """(filters, call_ids) pairs covering the predicates of filter_mask and its quirks."""
    at = some_timestamp(table)   # equal to a row's timestamp: the bounds are inclusive
    aware = at.replace(tzinfo=timezone.utc).astimezone(timezone(timedelta(hours=5, minutes=30)))
    F = rt.RetrieveFilters
    return [
        (None, None),
        (F(), None),
        (None, calls[:1]),                                    # filters=None: call_ids are not honoured
        (F(date_from=at), None),
        (F(date_to=at), None),
        (F(date_from=at - timedelta(hours=30), date_to=at), None),
        (F(date_from=aware), None),                           # timezone-aware bounds
        (F(date_from=at - timedelta(hours=1), date_to=aware), None),
        (F(), []),                                            # an empty list admits nothing
        (F(), calls[:2]),
        (F(), calls[-1:] + [UUID(int=7)]),                    # an id no row has
        (F(call_tags=["outage"]), None),
        (F(call_tags=["no-such-tag"]), None),
        (F(call_tags=["billing", "renewal"]), None),
        (F(call_tags=["outage"]), calls[: max(1, len(calls) // 2)]),       # call ids AND tags
        (F(call_tags=["billing"], date_from=at - timedelta(hours=50)), calls[1:]),
        (F(date_to=at + timedelta(hours=3), call_tags=["onboarding"]), []),
    ]


def host_packed(table, filters, call_ids):
    mask = table.filter_mask(filters, call_ids)
    return DenseIndex.pack_mask(np.ones(len(table), dtype=bool) if mask is None else mask)


def device_rule(table, batch):
    cols = fl.FilterColumns(table.call_started_at, table.call_ids)
    qset, lo, hi = fl.compile_predicates(cols, table.call_tags, batch)
    return filter_oracle.filter_masks(cols.started_us, cols.call_slot, cols.n_calls, qset, lo, hi, fl.mask_bytes(cols.n)), \
        (qset, lo, hi)


def test_the_two_forms_of_the_rule_agree():
    rng = np.random.default_rng(1)
    n, n_calls, nq = 77, 5, 9
    ts = rng.integers(-50, 50, n).astype(np.int64)
    ts[rng.random(n) < 0.3] = filter_oracle.I64_MIN
    slot = rng.integers(-1, n_calls + 1, n).astype(np.int32)       # -1 and n_calls: outside the dictionary
    lo = np.where(rng.random(nq) < 0.5, filter_oracle.I64_MIN, rng.integers(-30, 30, nq)).astype(np.int64)
    hi = np.where(rng.random(nq) < 0.5, filter_oracle.I64_MAX, rng.integers(-30, 30, nq)).astype(np.int64)
    for qset in (None, rng.integers(0, 1 << nq, n_calls).astype(np.uint64)):
        got = filter_oracle.filter_masks(ts, slot, n_calls, qset, lo, hi, 16)
        for q in range(nq):
            for i in range(128):
                want = i < n and filter_oracle.filter_bit(int(ts[i]), int(slot[i]), n_calls, qset, int(lo[q]), int(hi[q]), q)
                assert bool((got[q, i >> 3] >> (i & 7)) & 1) == bool(want), (q, i)


def test_filter_columns_number_the_calls_and_encode_nat():
    table, _ = make_table(np.random.default_rng(2), 40, n_calls=6)
    cols = fl.FilterColumns(table.call_started_at, table.call_ids)
    assert cols.n == 40 and cols.n_calls == len(set(table.call_ids)) == len(cols.slot_of)
    assert cols.started_us.dtype == np.int64 and cols.call_slot.dtype == np.int32
    assert sorted(cols.slot_of.values()) == list(range(cols.n_calls))
    assert all(cols.slot_of[c] == s for c, s in zip(table.call_ids, cols.call_slot))
    nat = np.isnat(table.call_started_at)
    assert nat.any() and np.all(cols.started_us[nat] == fl.NO_LOWER) and np.all(cols.started_us[~nat] != fl.NO_LOWER)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65, 200, 500])
def test_compiled_predicates_equal_the_host_mask(n):
    rng = np.random.default_rng(100 + n)
    table, calls = make_table(rng, n)
    for filters, call_ids in cases(table, calls):
        got, (qset, lo, hi) = device_rule(table, [(filters, call_ids)])
        assert np.array_equal(got[0], host_packed(table, filters, call_ids)), (filters, call_ids)
        assert fl.is_unfiltered(qset, lo, hi) == (table.filter_mask(filters, call_ids) is None)


def test_a_table_of_nat_rows_under_every_kind_of_bound():
    table, calls = make_table(np.random.default_rng(3), 70, nat_share=1.0)
    F = rt.RetrieveFilters
    for filters, expect_all in ((F(), True), (F(date_from=T0), False), (F(date_to=T0 + timedelta(days=99)), False),
                                (F(date_from=T0, date_to=T0 + timedelta(days=99)), False)):
        got, _ = device_rule(table, [(filters, None)])
        assert np.array_equal(got[0], host_packed(table, filters, None))
        assert bool(got.any()) == expect_all


def test_a_batch_of_64_mixed_queries_and_the_limit():
    rng = np.random.default_rng(4)
    table, calls = make_table(rng, 333, n_calls=23)
    pool = cases(table, calls)
    batch = [pool[int(i)] for i in rng.permutation(64) % len(pool)]
    got, (qset, lo, hi) = device_rule(table, batch)
    assert got.shape == (64, fl.mask_bytes(333)) and qset is not None and qset.dtype == np.uint64
    for q, (filters, call_ids) in enumerate(batch):
        assert np.array_equal(got[q], host_packed(table, filters, call_ids)), q
    cols = fl.FilterColumns(table.call_started_at, table.call_ids)
    with pytest.raises(ValueError, match="64"):
        fl.compile_predicates(cols, table.call_tags, batch + [pool[0]])
    # a batch without call scoping carries no call table at all
    assert fl.compile_predicates(cols, table.call_tags, [pool[0], pool[3], pool[5]])[0] is None


def test_compile_cost_is_in_calls_not_rows():
    """The compiled form of a request is the same arrays whether a call has one row or thousands."""
    calls = [UUID(int=1), UUID(int=2), UUID(int=3)]
    tags = {calls[0]: ["a"], calls[2]: ["a", "b"]}
    small = fl.FilterColumns(np.full(3, np.datetime64(T0, "us")), np.asarray(calls, dtype=object))
    big = fl.FilterColumns(np.full(3000, np.datetime64(T0, "us")), np.asarray(calls * 1000, dtype=object))
    batch = [(rt.RetrieveFilters(call_tags=["a"], date_from=T0), calls[1:]), (None, None)]
    for a, b in zip(fl.compile_predicates(small, tags, batch), fl.compile_predicates(big, tags, batch)):
        assert np.array_equal(a, b)


def test_argument_errors_are_codes_with_a_message(native_lib):
    fn = native_lib.crag_filter_masks_host
    i64 = np.zeros(64, dtype=np.int64)
    some = np.zeros(64, dtype=np.uint64)   # stands for a device pointer / a slot: an argument error comes before any use
    P = some.ctypes.data

    def call(started=P, slots=P, n_rows=100, n_calls=4, qset=P, lo=i64.ctypes.data, hi=i64.ctypes.data, nq=2, slot=P,
             out=P, stride=16):
        return fn(started, slots, n_rows, n_calls, qset, lo, hi, nq, slot, out, stride, None)

    bad = [dict(nq=0), dict(nq=65), dict(nq=-3), dict(n_rows=-1), dict(n_rows=1 << 31), dict(n_calls=-1),
           dict(stride=12), dict(stride=18), dict(stride=-4), dict(stride=0),
           dict(started=None), dict(slots=None), dict(lo=None), dict(hi=None), dict(slot=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) == -1, kw            # CRAG_EINVAL
        assert b"filter_masks_host" in native_lib.crag_last_error(), kw
    # an empty table with empty runs is nothing to do
    assert call(n_rows=0, stride=0, started=None, slots=None, out=None) == 0
