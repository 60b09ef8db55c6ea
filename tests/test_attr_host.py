"""Attribute filters, host side (no GPU): the two forms of the rule (tests/attr_oracle.py) agree; compile_attr_predicates
against hand-written cases; normalize_attr; DenseTable.filter_mask with entity, speaker and kind clauses; the entities
column stays aligned through add / insert / delete / delete_calls; the binding's constants, the gateway model and
_dense_has_scoping; the C entry refuses bad arguments with a code and a message before it touches the device."""
import re
from datetime import datetime, timedelta
from pathlib import Path
from uuid import UUID

import numpy as np
import pytest

from cadence_rag_amd import _native
from cadence_rag_amd import filters as fl
from cadence_rag_amd import retrieve as rt
from tests import attr_oracle

F = rt.RetrieveFilters
T0 = datetime(2024, 5, 1, 12, 0, 0)
CALLS = [UUID(int=i + 1) for i in range(4)]


# ---- the rule ---------------------------------------------------------------------------------------------------
def random_csr(rng, n, n_attrs, lo=-1):
    counts = rng.integers(0, 6, n)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = rng.integers(lo, n_attrs + 1, int(ptr[-1])).astype(np.int32)   # -1 and n_attrs: outside the dictionary
    return ptr, ids


def random_queries(rng, nq, n_attrs):
    return [[[int(k) for k in rng.integers(0, n_attrs, int(rng.integers(0, 4)))] for _ in range(int(rng.integers(0, 9)))]
            for _ in range(nq)]


def test_the_two_forms_of_the_rule_agree():
    rng = np.random.default_rng(1)
    for n, nq, n_attrs in ((0, 3, 5), (1, 1, 2), (77, 9, 12), (130, 64, 7)):
        ptr, ids = random_csr(rng, n, n_attrs)
        queries = random_queries(rng, nq, n_attrs)
        queries[0] = []
        stride = fl.mask_bytes(n) + 4
        shared = rng.integers(0, 256, stride, dtype=np.uint8)
        per_query = rng.integers(0, 256, (nq, stride + 4), dtype=np.uint8)
        keys, key_sets, clause_sets = attr_oracle.transpose(queries)
        assert np.all(np.diff(keys) > 0) and key_sets.shape == (keys.size, 8)
        for in_mask, in_stride in ((None, 0), (shared, 0), (per_query, stride + 4)):
            want = attr_oracle.attr_masks_direct(ptr, ids, n_attrs, queries, stride, in_mask, in_stride)
            got = attr_oracle.attr_masks(ptr, ids, n_attrs, keys, key_sets, clause_sets, nq, stride, in_mask, in_stride)
            assert np.array_equal(got, want), (n, nq, in_stride)
        # query 0 has no clause: without an input mask it admits exactly the rows below n
        ones = np.packbits(np.ones(n, dtype=bool), bitorder="little")
        open_run = attr_oracle.attr_masks(ptr, ids, n_attrs, keys, key_sets, clause_sets, nq, stride)[0]
        assert np.array_equal(open_run, np.pad(ones, (0, stride - ones.size)))


# ---- normalize_attr and the compiler ----------------------------------------------------------------------------
def test_normalize_attr():
    assert fl.normalize_attr("  Ada   LOVELACE\t\n") == "ada lovelace"
    assert fl.normalize_attr("Straße") == "strasse"                      # casefold, not lower
    assert fl.normalize_attr(None) is None and fl.normalize_attr("") is None and fl.normalize_attr("  \t ") is None
    assert fl.normalize_attr(42) == "42"
    assert fl.entity_namespace("  org ") == "entity:ORG"
    rows = fl.row_attributes(3, ["  Bob ", None, ""], None, [[("org", "ACME  Corp")], None, [{"label": "Person", "value": " ada "},
                                                                                                 ("person", None)]])
    assert rows == [[("speaker", "bob"), ("entity:ORG", "acme corp")], [], [("entity:PERSON", "ada")]]
    with pytest.raises(ValueError):
        fl.row_attributes(2, ["a"], None, None)


def columns_of(rows):
    return fl.AttributeColumns(rows)


def test_attribute_columns_number_by_first_appearance():
    cols = columns_of([[("speaker", "bob"), ("entity:ORG", "acme")], [], [("entity:ORG", "acme"), ("entity:ORG", "acme"),
                                                                            ("speaker", "ann")]])
    assert cols.id_of == {("speaker", "bob"): 0, ("entity:ORG", "acme"): 1, ("speaker", "ann"): 2} and cols.n_attrs == 3
    assert cols.attr_ptr.dtype == np.int64 and cols.attr_ptr.tolist() == [0, 2, 2, 5]
    assert cols.attr_ids.dtype == np.int32 and cols.attr_ids.tolist() == [0, 1, 1, 1, 2]      # duplicates are kept
    assert cols.n == 3 and cols.d_attr_ptr is None
    empty = columns_of([])
    assert empty.n == 0 and empty.attr_ptr.tolist() == [0] and empty.attr_ids.size == 0


def test_compile_attr_predicates_hand_written():
    cols = columns_of([[("speaker", "bob"), ("entity:ORG", "acme")], [("speaker", "ann"), ("entity:PERSON", "ada")],
                       [("kind", "summary")]])
    bob, acme, ann, ada, summary = 0, 1, 2, 3, 4
    batch = [
        # q0: the same key in two clauses of one query
        (F(entity_filters=[{"label": "org", "value": "ACME"}, {"label": " ORG ", "value": " acme "}]), None),
        # q1: no clauses at all (the call ids play no part)
        (F(call_tags=["x"]), [CALLS[0]]),
        # q2: `acme` at clause 1 where q0 has it at 0 and 1, `ada` at clause 0; speakers is the LAST clause (2)
        (F(entity_filters=[{"label": "person", "value": "Ada"}, {"label": "org", "value": "acme"}], speakers=["Bob", "ANN"]), None),
        # q3: an unknown key: the clause stays, without keys
        (F(entity_filters=[{"label": "org", "value": "nobody"}], kinds=["summary", "unknown-kind"]), None),
        (None, None),
    ]
    keys, key_sets, clause_sets = fl.compile_attr_predicates(cols, batch)
    assert keys.dtype == np.int32 and keys.tolist() == [bob, acme, ann, ada, summary]
    assert key_sets.dtype == np.uint64 and key_sets.shape == (5, 8) and clause_sets.dtype == np.uint64
    want_sets = np.zeros((5, 8), dtype=np.uint64)
    want_sets[acme, 0] = 1 << 0
    want_sets[acme, 1] = (1 << 0) | (1 << 2)
    want_sets[ada, 0] = 1 << 2
    want_sets[bob, 2] = want_sets[ann, 2] = 1 << 2
    want_sets[summary, 1] = 1 << 3
    assert np.array_equal(key_sets, want_sets)
    assert clause_sets.tolist() == [0b1101, 0b1101, 0b0100, 0, 0, 0, 0, 0]
    # and the arrays mean what the clause lists mean
    queries = [[[acme], [acme]], [], [[ada], [acme], [bob, ann]], [[], [summary]], []]
    assert all(np.array_equal(a, b) for a, b in zip(attr_oracle.transpose(queries), (keys, key_sets, clause_sets)))
    # no query with a clause: nothing to run
    assert fl.compile_attr_predicates(cols, [(F(date_from=T0), None), (None, [CALLS[0]]), (F(speakers=[], kinds=None), None)]) is None
    # query 63 keeps its bit
    last = fl.compile_attr_predicates(cols, [(None, None)] * 63 + [(F(kinds=["summary"]), None)])
    assert last[0].tolist() == [summary] and int(last[1][0, 0]) == 1 << 63 and int(last[2][0]) == 1 << 63
    with pytest.raises(ValueError, match="64"):
        fl.compile_attr_predicates(cols, [(None, None)] * 65)


def test_nine_clauses_are_refused():
    cols = columns_of([[("entity:ORG", "acme")]])
    eight = [{"label": "org", "value": f"v{i}"} for i in range(8)]
    assert fl.compile_attr_predicates(cols, [(F(entity_filters=eight), None)])[2].tolist() == [1] * 8
    with pytest.raises(ValueError, match="8"):
        fl.compile_attr_predicates(cols, [(F(entity_filters=eight[:7], speakers=["a"], kinds=["b"]), None)])
    with pytest.raises(ValueError, match="8"):
        fl.attr_clauses(F(entity_filters=eight + eight[:1]))


def test_compile_cost_is_in_keys_not_rows():
    rows = [[("speaker", "bob")], [("speaker", "ann"), ("entity:ORG", "acme")]]
    batch = [(F(speakers=["ann"], entity_filters=[("org", "acme")]), None), (F(kinds=["x"]), None)]
    small, big = columns_of(rows), columns_of(rows * 1000)
    for a, b in zip(fl.compile_attr_predicates(small, batch), fl.compile_attr_predicates(big, batch)):
        assert np.array_equal(a, b)


# ---- DenseTable.filter_mask -------------------------------------------------------------------------------------
class _Rows:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def bare_table(columns, entities, started=None, tags=None):
    """A DenseTable without an index: filter_mask reads the host columns and len() only."""
    n = len(columns["call_id"])
    table = object.__new__(rt.DenseTable)
    table.index = _Rows(n)
    table.columns = {k: list(v) for k, v in columns.items()}
    table.call_ids = np.asarray(columns["call_id"], dtype=object)
    table.call_started_at = np.asarray(started if started is not None else [np.datetime64("NaT")] * n, dtype="datetime64[us]")
    table.call_tags = tags or {}
    table.entities = entities
    return table


SPEAKERS = ["Bob", "ann", "BOB ", None, "Cy", "ann"]
ENTITIES = [[("org", "Acme"), ("person", "Ada")], [("ORG", "acme")], [("person", "ada"), {"label": "org", "value": "Initech"}],
            [("org", "acme"), ("person", "ada")], [], [("product", "acme")]]


def chunk_table():
    return bare_table({"chunk_id": list(range(6)), "call_id": [CALLS[i % 3] for i in range(6)], "speaker": SPEAKERS}, ENTITIES,
                      started=[np.datetime64(T0 + timedelta(hours=i), "us") for i in range(6)],
                      tags={CALLS[0]: ["billing"], CALLS[1]: ["outage"]})


def test_filter_mask_attribute_semantics():
    t = chunk_table()
    mask = lambda f, c=None: t.filter_mask(f, c).tolist()
    yes, no = True, False
    # one entity filter; label and value in normal form on both sides; the label is part of the key
    assert mask(F(entity_filters=[{"label": "org", "value": " ACME "}])) == [yes, yes, no, yes, no, no]
    # AND across entity filters
    assert mask(F(entity_filters=[{"label": "org", "value": "acme"}, {"label": "Person", "value": "Ada"}])) == [yes, no, no, yes, no, no]
    # OR inside speakers; a row without a speaker passes no speakers clause
    assert mask(F(speakers=["bob", "CY"])) == [yes, no, yes, no, yes, no]
    assert mask(F(speakers=["ann"], entity_filters=[("org", "acme")])) == [no, yes, no, no, no, no]
    # an unknown value, and a value that is no attribute: the clause admits nothing
    assert mask(F(entity_filters=[{"label": "org", "value": "nobody"}])) == [no] * 6
    assert mask(F(speakers=[""])) == [no] * 6
    # the NULL namespace: this table has no `kind` column
    assert mask(F(kinds=["summary"])) == [no] * 6
    # falsy fields are not applied
    assert t.filter_mask(F(speakers=[], kinds=None, entity_filters=[]), None) is None
    assert t.filter_mask(None, None) is None
    # intersection with dates, call ids and tags
    assert mask(F(entity_filters=[("org", "acme")], date_from=T0 + timedelta(hours=1))) == [no, yes, no, yes, no, no]
    assert mask(F(entity_filters=[("org", "acme")]), [CALLS[0]]) == [yes, no, no, yes, no, no]
    assert mask(F(entity_filters=[("org", "acme")], call_tags=["outage"])) == [no, yes, no, no, no, no]
    assert mask(F(speakers=["bob"], call_tags=["billing"], date_to=T0), [CALLS[0], CALLS[1]]) == [yes, no, no, no, no, no]
    # entities never tracked: NULL, where an empty tracked list is merely empty -- both admit nothing
    t.entities = None
    assert mask(F(entity_filters=[("org", "acme")])) == [no] * 6 and mask(F(speakers=["ann"])) == [no, yes, no, no, no, yes]
    # the artifact table: `kind` and no `speaker`, so a speakers filter returns no artifact rows
    arts = bare_table({"artifact_chunk_id": [0, 1, 2], "call_id": CALLS[:3], "kind": ["Summary", "notes", None]},
                      [[("org", "acme")], [], []])
    assert arts.filter_mask(F(kinds=["summary", "transcript"]), None).tolist() == [yes, no, no]
    assert arts.filter_mask(F(speakers=["bob"]), None).tolist() == [no, no, no]
    assert arts.filter_mask(F(kinds=["notes", "summary"], entity_filters=[("org", "acme")]), None).tolist() == [yes, no, no]


def test_the_compiled_rule_equals_filter_mask():
    """compile_attr_predicates + the numpy rule of the kernel == pack_mask(filter_mask) for the attribute part."""
    from cadence_rag_amd.dense_index import DenseIndex
    t = chunk_table()
    cols = fl.AttributeColumns(t._row_attrs())
    batch = [(F(entity_filters=[("org", "acme")]), None), (F(speakers=["bob", "cy"]), None), (F(kinds=["x"]), None),
             (F(speakers=["ann"], entity_filters=[("org", "acme"), ("person", "ada")]), None),
             (F(entity_filters=[("org", "acme"), ("person", "ada")]), None)]
    keys, key_sets, clause_sets = fl.compile_attr_predicates(cols, batch)
    got = attr_oracle.attr_masks(cols.attr_ptr, cols.attr_ids, cols.n_attrs, keys, key_sets, clause_sets, len(batch), 4)
    for q, (f, c) in enumerate(batch):
        assert np.array_equal(got[q], DenseIndex.pack_mask(t.filter_mask(f, c))), q


def test_scoped_positions_leaves_attribute_requests_to_the_masked_scan():
    t = chunk_table()
    assert t.scoped_positions(F(), [CALLS[0]], 100).tolist() == [0, 3]
    assert t.scoped_positions(F(speakers=["bob"]), [CALLS[0]], 100) is None
    assert t.scoped_positions(F(entity_filters=[("org", "acme")]), [CALLS[0]], 100) is None
    assert t.scoped_positions(F(kinds=["x"]), [CALLS[0]], 100) is None


# ---- the entities column through the edits ----------------------------------------------------------------------
class FakeIndex:
    """Stands for DenseIndex where only the bookkeeping of the host columns is under test."""

    def __init__(self, dim, capacity=1 << 16, device=0):
        self.dim, self.capacity, self.device, self.ids = dim, capacity, device, []

    def __len__(self):
        return len(self.ids)

    def add(self, vectors, ids=None):
        self.ids.extend(int(i) for i in ids)

    def insert(self, vectors, ids):
        self.ids = sorted(self.ids + [int(i) for i in ids])

    def remove(self, ids):
        gone = set(int(i) for i in ids)
        before = len(self.ids)
        self.ids = [i for i in self.ids if i not in gone]
        return before - len(self.ids)

    def compact(self, keep):
        self.ids = [i for i, k in zip(self.ids, keep) if k]
        return len(self.ids)

    def close(self):
        pass


def ents_of(i):
    return [("org", f"org-{i % 3}"), {"label": "ticket", "value": f"T-{i}"}]


def rows_for(ids, with_entities=True):
    ids = list(ids)
    cols = {"chunk_id": ids, "call_id": [CALLS[i % 4] for i in ids], "speaker": [f"s{i % 2}" for i in ids]}
    if with_entities:
        cols["entities"] = [ents_of(i) for i in ids]
    return cols


def assert_aligned(table, bare=()):
    ids = table.columns["chunk_id"]
    assert len(table.entities) == len(table) == len(ids) and "entities" not in table.columns
    for i, ents in zip(ids, table.entities):
        assert ents == ([] if i in bare else [("org", f"org-{i % 3}"), ("ticket", f"T-{i}")]), i
    # and the rule sees them at the right rows
    want = [i for i in ids if i % 3 == 1 and i not in bare]
    got = table.filter_mask(F(entity_filters=[{"label": "ORG", "value": "ORG-1"}]), None)
    assert [i for i, k in zip(ids, got) if k] == want
    one = ids[len(ids) // 2]
    got = table.filter_mask(F(entity_filters=[("ticket", f"t-{one}")], speakers=[f"S{one % 2}"]), None)
    assert [i for i, k in zip(ids, got) if k] == ([] if one in bare else [one])


def test_entities_stay_aligned_through_add_insert_delete(monkeypatch):
    monkeypatch.setattr(rt, "DenseIndex", FakeIndex)
    vec = lambda n: np.zeros((n, 4), dtype=np.float32)
    table = rt.DenseTable("chunks", "chunk_id", dim=4, capacity=64, device=0)   # (growing moves rows on the device)
    table.add(vec(5), rows_for(range(10, 15), with_entities=False))
    assert table.entities is None                                     # not tracked yet: NULL
    assert not table.filter_mask(F(entity_filters=[("org", "org-1")]), None).any()
    table.add(vec(5), rows_for(range(20, 25)))                        # tracked from the first batch that carries them
    bare = set(range(10, 15))
    assert_aligned(table, bare)
    table.add(vec(3), rows_for(range(30, 33), with_entities=False))   # a batch without them contributes []
    bare |= set(range(30, 33))
    assert_aligned(table, bare)
    table.insert(vec(4), rows_for([40, 3, 17, 26]))                   # ids below the stored ones: merged in id order
    assert table.columns["chunk_id"] == sorted(table.columns["chunk_id"])
    assert_aligned(table, bare)
    table.insert(vec(2), rows_for([16, 5], with_entities=False))
    bare |= {16, 5}
    assert_aligned(table, bare)
    assert table.delete([3, 22, 31, 999]) == 3
    assert_aligned(table, bare)
    assert table.delete_calls([CALLS[1]]) > 0
    assert all(c != CALLS[1] for c in table.call_ids)
    assert_aligned(table, bare)
    sink = table.sink(lambda ids: rows_for(ids))
    sink.add(vec(2), [50, 7])
    assert_aligned(table, bare)
    with pytest.raises(ValueError, match="entities"):
        table.add(vec(2), dict(rows_for([60, 61]), entities=[[]]))


def test_a_table_that_never_sees_entities_tracks_nothing(monkeypatch):
    monkeypatch.setattr(rt, "DenseIndex", FakeIndex)
    table = rt.DenseTable("chunks", "chunk_id", dim=4, capacity=8, device=0)
    table.add(np.zeros((3, 4), dtype=np.float32), rows_for([1, 2, 3], with_entities=False))
    table.insert(np.zeros((1, 4), dtype=np.float32), rows_for([0], with_entities=False))
    table.delete([2])
    assert table.entities is None and table._attr_cols is None


# ---- binding, gateway, planner ----------------------------------------------------------------------------------
def test_native_constants_equal_the_headers():
    text = (Path(__file__).resolve().parent.parent / "include" / "crag_dense.h").read_text()
    for name in ("CRAG_ATTR_MAX_QUERIES", "CRAG_ATTR_MAX_CLAUSES", "CRAG_ATTR_MAX_KEYS"):
        assert int(re.search(rf"#define {name}\s+(\d+)", text).group(1)) == getattr(_native, name), name
    assert int(re.search(r"#define CRAG_E2BIG \((-\d+)\)", text).group(1)) == _native.CRAG_E2BIG
    assert (fl.MAX_CLAUSES, fl.MAX_KEYS) == (8, 512) and attr_oracle.MAX_CLAUSES == fl.MAX_CLAUSES
    assert len(_native.SIGNATURES["crag_attr_masks_host"][1]) == 15


def test_gateway_model_round_trips_the_fields():
    from cadence_rag_amd import gateway
    payload = {"entity_filters": [{"label": "ORG", "value": "Acme"}], "speakers": ["Bob"], "kinds": ["summary"],
               "call_tags": ["billing"]}
    model = gateway.RetrieveFiltersModel(**payload)
    filters = rt.RetrieveFilters(**model.model_dump())
    assert filters.entity_filters == payload["entity_filters"] and filters.speakers == ["Bob"] and filters.kinds == ["summary"]
    assert filters.call_tags == ["billing"]
    blank = rt.RetrieveFilters(**gateway.RetrieveFiltersModel().model_dump())
    assert blank == rt.RetrieveFilters() and blank.entity_filters is None and blank.speakers is None and blank.kinds is None


def test_dense_has_scoping_counts_the_attribute_fields():
    assert rt._dense_has_scoping(F(entity_filters=[{"label": "org", "value": "acme"}]), None)
    assert rt._dense_has_scoping(F(speakers=["bob"]), None) and rt._dense_has_scoping(F(kinds=["summary"]), None)
    assert not rt._dense_has_scoping(F(speakers=[], kinds=[], entity_filters=[]), None)
    assert not rt._dense_has_scoping(F(), None) and not rt._dense_has_scoping(None, None)


# ---- the C entry's argument checks ------------------------------------------------------------------------------
def test_argument_errors_are_codes_with_a_message(native_lib):
    fn = native_lib.crag_attr_masks_host
    some = np.zeros(64, dtype=np.uint64)   # stands for a device pointer / a slot: an argument error comes before any use
    P = some.ctypes.data
    keys = np.asarray([1, 5, 9], dtype=np.int32)
    key_sets = np.zeros((3, 8), dtype=np.uint64)
    key_sets[:, 0] = 0b01
    key_sets[1, 1] = 0b10
    clause_sets = np.asarray([0b01, 0b10, 0, 0, 0, 0, 0, 0], dtype=np.uint64)

    def call(ptr=P, ids=P, n_rows=100, n_attrs=10, keys=keys, key_sets=key_sets, n_keys=3, clause_sets=clause_sets, nq=2,
             in_mask=None, in_stride=0, slot=P, out=P, stride=16):
        k = None if keys is None else np.ascontiguousarray(keys, dtype=np.int32)
        s = None if key_sets is None else np.ascontiguousarray(key_sets, dtype=np.uint64)
        c = None if clause_sets is None else np.ascontiguousarray(clause_sets, dtype=np.uint64)
        return fn(ptr, ids, n_rows, n_attrs, None if k is None else k.ctypes.data, None if s is None else s.ctypes.data,
                  n_keys, None if c is None else c.ctypes.data, nq, in_mask, in_stride, slot, out, stride, None)

    not_subset = key_sets.copy()
    not_subset[0, 1] = 0b01                          # query 0 has no clause 1
    high_bit = clause_sets.copy()
    high_bit[0] |= 0b100                             # a bit at nq
    high_key_bit = key_sets.copy()
    high_key_bit[2, 0] |= 1 << 40
    bad = [dict(nq=0), dict(nq=65), dict(nq=-3), dict(n_rows=-1), dict(n_rows=1 << 31), dict(n_attrs=-1), dict(n_keys=-1),
           dict(keys=[1, 1, 9]), dict(keys=[5, 1, 9]), dict(keys=[-1, 5, 9]), dict(keys=[1, 5, 10]),
           dict(clause_sets=high_bit), dict(key_sets=high_key_bit), dict(key_sets=not_subset),
           dict(stride=12), dict(stride=18), dict(stride=-4), dict(stride=0),
           dict(in_mask=P, in_stride=12), dict(in_mask=P, in_stride=18), dict(in_mask=P, in_stride=-4), dict(in_mask=P + 2),
           dict(out=P + 1), dict(out=P + 2),
           dict(ptr=None), dict(ids=None), dict(keys=None), dict(key_sets=None), dict(clause_sets=None), dict(slot=None),
           dict(out=None)]
    for kw in bad:
        assert call(**kw) == -1, kw            # CRAG_EINVAL
        assert b"attr_masks_host" in native_lib.crag_last_error(), kw
    # more keys than a call takes: the caller splits
    many = np.arange(513, dtype=np.int32)
    sets = np.zeros((513, 8), dtype=np.uint64)
    sets[:, 0] = 1
    assert call(keys=many, key_sets=sets, n_keys=513, n_attrs=600) == _native.CRAG_E2BIG == -5
    assert b"attr_masks_host" in native_lib.crag_last_error()
    # an empty table with empty runs is nothing to do
    assert call(n_rows=0, stride=0, ptr=None, ids=None, out=None) == 0


# ---- the batch splitter of AttributeColumns.masks and FacetColumns.counts ---------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 3, 64])
def test_halving_on_e2big_tiles_the_batch_in_order(nq):
    """A fake entry that answers CRAG_E2BIG above a width: the slices it accepts tile [0, nq) in order without overlap,
    every refused slice is retried as its halves and never as itself, and a single query that is too big raises the
    caller's ValueError at that query, behind the slices in front of it."""
    def too_big(q):
        return ValueError(f"query {q} is too big")

    for width in (1, 2, 5, 64):
        issued, accepted = [], []

        def call(q0, n):
            issued.append((q0, n))
            if n > width:
                return _native.CRAG_E2BIG
            accepted.append((q0, n))
            return 0

        assert fl._halve_on_e2big(call, 0, nq, too_big) is None
        at = 0
        for q0, n in accepted:
            assert q0 == at and 1 <= n <= width, (nq, width, accepted)
            at += n
        assert at == nq and issued[0] == (0, nq) and len(set(issued)) == len(issued), (nq, width, issued)
    for heavy in sorted({0, nq // 2, nq - 1}):
        accepted = []

        def refusing(q0, n):
            if q0 <= heavy < q0 + n:
                return _native.CRAG_E2BIG
            accepted.append((q0, n))
            return 0

        with pytest.raises(ValueError, match=f"query {heavy} is too big"):
            fl._halve_on_e2big(refusing, 0, nq, too_big)
        assert [q for q0, n in accepted for q in range(q0, q0 + n)] == list(range(heavy)), (nq, heavy, accepted)
