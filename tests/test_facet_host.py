"""Facet counts, the host side: the layout of FacetColumns, the host rule against the oracle, the argument
checks of crag_facet_counts_host (they come before any HIP call, so they run without a GPU), the request fields and the
response key."""
import re
from pathlib import Path

import numpy as np
import pytest

from cadence_rag_amd import _native
from cadence_rag_amd import filters as fl
from cadence_rag_amd import retrieve as rt
from tests import facet_oracle


def random_rows(rng, n, n_entities=40):
    speakers = [None if rng.random() < 0.1 else f"speaker {int(rng.integers(5))}" for _ in range(n)]
    kinds = [f"Kind{int(rng.integers(3))}" for _ in range(n)]
    entities = []
    for _ in range(n):
        listed = [("service" if rng.random() < 0.7 else "Ticket", f"v{int(rng.zipf(1.5)) % n_entities}")
                  for _ in range(int(rng.integers(0, 5)))]
        entities.append(listed + listed[:1])   # the first entity twice: a duplicate inside the row
    return fl.row_attributes(n, speakers, kinds, entities)


NAMES = ["speaker", "kind", "entity:SERVICE", "entity:TICKET", "entity:ABSENT"]


# ---- FacetColumns -----------------------------------------------------------------------------------------------
def check_layout(rows):
    attrs = fl.AttributeColumns(rows)
    cols = fl.FacetColumns(attrs)
    assert cols.n == len(rows) and cols.n_attrs == attrs.n_attrs == len(cols.facet_keys)
    assert cols.facet_keys == sorted(attrs.id_of)                       # facet ids ordered by (namespace, value)
    spaces = sorted({ns for ns, _ in cols.facet_keys})
    assert sorted(cols.ranges) == spaces
    at = 0
    for ns in spaces:                                                   # contiguous, complete, in namespace order
        lo, hi = cols.ranges[ns]
        assert lo == at and hi > lo and all(k[0] == ns for k in cols.facet_keys[lo:hi])
        at = hi
    assert at == cols.n_attrs
    assert cols.post_ptr.dtype == np.int64 and cols.post_ptr.shape == (cols.n_attrs + 1,) and cols.post_ptr[0] == 0
    assert cols.post_rows.dtype == np.int32 and cols.post_fid.dtype == np.int32
    assert cols.post_ptr[-1] == cols.n_postings == cols.post_rows.size == cols.post_fid.size
    for fid, key in enumerate(cols.facet_keys):
        mine = cols.post_rows[cols.post_ptr[fid]:cols.post_ptr[fid + 1]]
        assert np.all(np.diff(mine) > 0)                                # ascending, each row once
        assert list(mine) == [i for i, r in enumerate(rows) if key in r]
        assert np.all(cols.post_fid[cols.post_ptr[fid]:cols.post_ptr[fid + 1]] == fid)
    return cols


def test_layout_of_random_tables():
    rng = np.random.default_rng(3)
    for n in (1, 7, 200):
        cols = check_layout(random_rows(rng, n))
    assert cols.n_postings < fl.AttributeColumns(random_rows(np.random.default_rng(3), 1)).attr_ids.size + 10 ** 6


def test_in_row_duplicates_are_stored_once():
    rows = [[("kind", "a")] * 5 + [("kind", "b")], [("kind", "b"), ("kind", "b")]]
    cols = check_layout(rows)
    assert fl.AttributeColumns(rows).attr_ids.size == 8 and cols.n_postings == 3
    assert list(cols.post_rows) == [0, 0, 1] and list(cols.post_fid) == [0, 1, 1]


def test_numbering_does_not_depend_on_row_order():
    rng = np.random.default_rng(11)
    rows = random_rows(rng, 150)
    order = rng.permutation(len(rows))
    a, b = fl.FacetColumns(fl.AttributeColumns(rows)), fl.FacetColumns(fl.AttributeColumns([rows[i] for i in order]))
    assert list(fl.AttributeColumns(rows).id_of) != list(fl.AttributeColumns([rows[i] for i in order]).id_of)
    assert a.facet_keys == b.facet_keys and a.ranges == b.ranges and np.array_equal(a.post_ptr, b.post_ptr)


def test_an_empty_table_and_a_table_without_attributes():
    for rows in ([], [[], [], []]):
        cols = check_layout(rows)
        assert cols.n_attrs == 0 and cols.n_postings == 0 and cols.ranges == {} and list(cols.post_ptr) == [0]
        lo, hi = cols.requested(["speaker", "entity:x"])
        assert list(lo) == [0, 0] and list(hi) == [0, 0]


def test_requested_ranges_and_their_limits():
    cols = fl.FacetColumns(fl.AttributeColumns([[("entity:SERVICE", "api"), ("speaker", "bob")], [("speaker", "al")]]))
    lo, hi = cols.requested(["speaker", "entity:service", "kind"])
    assert list(zip(lo, hi)) == [(1, 3), (0, 1), (0, 0)] and lo.dtype == np.int32
    assert fl.facet_namespace(" Entity: service ") == "entity:SERVICE" and fl.facet_namespace("kind") == "kind"
    with pytest.raises(ValueError, match="at most 16"):
        cols.requested([f"entity:L{i}" for i in range(17)])
    with pytest.raises(ValueError, match="once"):
        cols.requested(["speaker", "speaker"])


# ---- the host rule ----------------------------------------------------------------------------------------------
def test_facets_host_equals_the_oracle():
    rng = np.random.default_rng(5)
    some = 0
    for n in (0, 1, 33, 400):
        rows = random_rows(rng, n)
        for bits in (None, np.zeros(n, dtype=bool), np.ones(n, dtype=bool), rng.random(n) < 0.4):
            for top in (1, 3, 64):
                got = fl.facets_host(rows, bits, NAMES, top)
                want = facet_oracle.facets(rows, bits, NAMES, top)
                assert got == want, (n, top)
                some += sum(distinct > top for _, distinct in got[1].values())
    assert some > 10                                                    # lists were cut
    with pytest.raises(ValueError):
        fl.facets_host([], None, NAMES, 0)
    with pytest.raises(ValueError):
        fl.facets_host([], None, NAMES, 65)


def test_ties_go_by_value_and_names_are_reported_as_given():
    rows = [[("entity:SERVICE", "zeta")], [("entity:SERVICE", "alpha")], [("entity:SERVICE", "mid"), ("entity:SERVICE", "mid")]]
    rows_seen, out = fl.facets_host(rows, None, ["entity:service"], 2)
    assert rows_seen == 3 and out == {"entity:service": ([("alpha", 1), ("mid", 1)], 3)}


# ---- binding ----------------------------------------------------------------------------------------------------
def test_native_constants_equal_the_header():
    text = (Path(__file__).resolve().parent.parent / "include" / "crag_dense.h").read_text()
    for name in ("CRAG_FACET_MAX_QUERIES", "CRAG_FACET_MAX_NAMESPACES", "CRAG_FACET_MAX_TOP"):
        assert int(re.search(rf"#define {name}\s+(\d+)", text).group(1)) == getattr(_native, name), name
    assert (fl.MAX_FACET_NAMESPACES, fl.MAX_FACET_TOP) == (16, 64)
    assert len(_native.SIGNATURES["crag_facet_counts_host"][1]) == 20


def test_argument_errors_come_before_any_hip_call(native_lib):
    fn = native_lib.crag_facet_counts_host
    some = np.zeros(64, dtype=np.uint64)   # stands for device pointers: an argument error comes before any use
    P = some.ctypes.data

    def call(ptr=P, rows=P, fid=P, n_postings=50, n_rows=100, n_attrs=10, masks=P, stride=16, lo=(0, 4), hi=(4, 10),
             n_ranges=None, nq=2, top=5, work=P, work_bytes=None, ids=P, counts=P, distinct=P, out_rows=P):
        l = None if lo is None else np.ascontiguousarray(lo, dtype=np.int32)
        h = None if hi is None else np.ascontiguousarray(hi, dtype=np.int32)
        r = (0 if l is None else int(l.size)) if n_ranges is None else n_ranges
        if work_bytes is None:
            width = 0 if l is None or h is None else int(np.maximum(h.astype(np.int64) - l, 0).sum())
            work_bytes = max(native_lib.crag_facet_workspace_bytes(max(n_rows, 0), max(nq, 0), width, 1), 0)
        return fn(ptr, rows, fid, n_postings, n_rows, n_attrs, masks, stride, None if l is None else l.ctypes.data,
                  None if h is None else h.ctypes.data, r, nq, top, work, work_bytes, ids, counts, distinct, out_rows, None)

    seventeen = (list(range(17)), list(range(1, 18)))
    bad = [dict(nq=0), dict(nq=65), dict(top=0), dict(top=65),
           dict(lo=seventeen[0], hi=seventeen[1], n_attrs=20), dict(n_ranges=-1),
           dict(lo=(0, 4), hi=(4, 11)), dict(lo=(-1, 4), hi=(4, 10)), dict(lo=(5, 6), hi=(4, 10)),      # outside, lo > hi
           dict(lo=(0, 3), hi=(4, 10)), dict(lo=(2, 0), hi=(3, 10)), dict(lo=(0, 0), hi=(4, 4)),             # overlapping
           dict(masks=P + 2), dict(masks=P + 1), dict(stride=12), dict(stride=18), dict(stride=-4),
           dict(n_rows=-1), dict(n_rows=1 << 31), dict(n_attrs=-1), dict(n_postings=-1),
           dict(ids=None), dict(counts=None), dict(distinct=None), dict(out_rows=None),
           dict(lo=None, n_ranges=2), dict(hi=None, n_ranges=2), dict(ptr=None), dict(rows=None), dict(fid=None),
           dict(work=None), dict(work=P + 4), dict(work_bytes=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw            # CRAG_EINVAL
        assert b"facet_counts_host" in native_lib.crag_last_error(), kw
    # the workspace one byte short: the caller splits the batch
    need = native_lib.crag_facet_workspace_bytes(100, 2, 10, 1)
    assert need == 100 * 8 + 2 * 10 * 4
    assert call(work_bytes=need - 1) == _native.CRAG_E2BIG == -5
    assert b"facet_counts_host" in native_lib.crag_last_error()
    assert call(masks=None, stride=0, work_bytes=2 * 10 * 4 - 1) == _native.CRAG_E2BIG      # no masks: no query sets
    assert native_lib.crag_facet_workspace_bytes(100, 2, 10, 0) == 80 and native_lib.crag_facet_workspace_bytes(-1, 2, 10, 0) == -1


# ---- the request and the response -------------------------------------------------------------------------------
def test_retrieve_request_validates_the_facet_fields():
    assert rt.RetrieveRequest(query="q").facets is None and rt.RetrieveRequest(query="q").facet_top == 10
    rt.RetrieveRequest(query="q", facets=["kind"] * 16, facet_top=64)
    rt.RetrieveRequest(query="q", facets=[], facet_top=1)
    for kw in (dict(facet_top=0), dict(facet_top=65), dict(facets=["kind"] * 17)):
        with pytest.raises(ValueError):
            rt.RetrieveRequest(query="q", **kw)


def test_the_gateway_model_carries_and_rejects():
    from pydantic import ValidationError

    from cadence_rag_amd import gateway
    model = gateway.RetrieveRequestModel(query="q", facets=["speaker", "entity:SERVICE"], facet_top=3)
    assert model.facets == ["speaker", "entity:SERVICE"] and model.facet_top == 3
    blank = gateway.RetrieveRequestModel(query="q")
    assert blank.facets is None and blank.facet_top == 10
    for kw in (dict(facet_top=0), dict(facet_top=65), dict(facets=["kind"] * 17)):
        with pytest.raises(ValidationError):
            gateway.RetrieveRequestModel(query="q", **kw)


class StubBackend(rt.RetrieveBackend):
    def __init__(self):
        self.asked = []

    def fetch_chunks_bm25(self, query, filters, call_ids, limit):
        return [{"chunk_id": 7, "call_id": "c", "speaker": "bob", "start_ts_ms": 0, "end_ts_ms": 1, "text": "hello", "score": 1.0}]

    def facets(self, table_name, filters, call_ids, namespaces, top):
        self.asked.append((table_name, filters, call_ids, tuple(namespaces), top))
        return {"rows": 3, "facets": {ns: {"values": [{"value": table_name, "count": 3}], "distinct": 1} for ns in namespaces}}


@pytest.mark.parametrize("style", ["evidence_pack_json", "ids_only"])
@pytest.mark.parametrize("query", ["hello", "   "])
def test_the_facets_key_is_present_exactly_when_requested(monkeypatch, style, query):
    from cadence_rag_amd import embeddings
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: False)
    be = StubBackend()

    def ask(**kw):
        resp = rt.retrieve_evidence(rt.RetrieveRequest(query=query, return_style=style, **kw), be)
        resp.pop("query_id")
        return resp

    plain = ask()
    assert "facets" not in plain and "facets" not in ask(facets=[]) and "facets" not in ask(facets=None) and not be.asked
    filters = rt.RetrieveFilters(speakers=["bob"])
    with_facets = ask(facets=["speaker", "entity:SERVICE"], facet_top=4, filters=filters)
    assert [a[0] for a in be.asked] == ["chunks", "artifact_chunks"]
    assert all(a[1:] == (filters, None, ("speaker", "entity:SERVICE"), 4) for a in be.asked)
    got = with_facets.pop("facets")
    assert set(got) == {"chunks", "artifact_chunks"} and got["chunks"]["rows"] == 3
    assert got["artifact_chunks"]["facets"]["entity:SERVICE"] == {"values": [{"value": "artifact_chunks", "count": 3}], "distinct": 1}
    assert with_facets == ask(filters=filters)                       # the rest of the response is the unrequested one
    assert rt.RetrieveBackend().facets("chunks", None, None, ["kind"], 5) == {}
