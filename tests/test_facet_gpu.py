"""Facet counts on the GPU (crag_facet_counts_host) against tests/facet_oracle.py and the host rule
filters.facets_host.  Every comparison is == on integers and strings.  The kernel's geometry the shapes aim at: 64-row
groups and 1024-row spans in the mask transpose, chunks of 4096 postings in the count, 256-entry tiles and a 512-key
buffer in the selection."""
from datetime import datetime, timedelta
from uuid import UUID

import numpy as np
import pytest
import torch

import facet_oracle
from cadence_rag_amd import embeddings
from cadence_rag_amd import filters as fl
from cadence_rag_amd import retrieve as rt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAMES = ["speaker", "kind", "entity:SERVICE", "entity:TICKET", "entity:ABSENT"]


def random_rows(rng, n, n_entities=300):
    speakers = [None if rng.random() < 0.1 else f"speaker {int(rng.integers(8))}" for _ in range(n)]
    kinds = [f"kind {int(rng.integers(6))}" for _ in range(n)]
    entities = []
    for _ in range(n):
        listed = [("service" if rng.random() < 0.7 else "ticket", f"v{int(rng.zipf(1.3)) % n_entities:04d}")
                  for _ in range(int(rng.integers(0, 4)))]
        entities.append(listed + listed[:1])   # the first entity twice: a duplicate inside the row
    return fl.row_attributes(n, speakers, kinds, entities)


def columns(rows):
    return fl.FacetColumns(fl.AttributeColumns(rows), device=DEV)


def pack(bits, stride=None, junk=True):
    """bool [nq, n] as device masks [nq, stride]; with `junk` every bit at and beyond n is SET (it must not count)."""
    nq, n = bits.shape
    stride = fl.mask_bytes(n) if stride is None else stride
    wide = np.full((nq, stride * 8), bool(junk))
    wide[:, :n] = bits
    return torch.from_numpy(np.packbits(wide, axis=1, bitorder="little")).to(DEV)


def mask_set(rng, nq, n):
    """One different mask per query: all zero, all one and random ones of several densities."""
    bits = np.zeros((nq, n), dtype=bool)
    for q in range(nq):
        bits[q] = {0: np.zeros(n, bool), 1: np.ones(n, bool)}.get(q % 7, rng.random(n) < (0.03 + 0.9 * ((q * 37) % 11) / 11))
    return bits


def answer(cols, names, out):
    """The device tensors of FacetColumns.counts in the oracle's shape, per query; also checks the padding."""
    ids, counts, distinct, rows = (t.cpu().numpy() for t in out)
    assert ids.dtype == np.int32 and distinct.dtype == np.int32 and rows.dtype == np.int64
    assert np.array_equal(ids < 0, counts == 0) and np.all(ids[ids < 0] == -1)
    got = []
    for q in range(rows.shape[0]):
        per = {}
        for r, ns in enumerate(names):
            live = ids[q, r] >= 0
            assert not live[np.argmin(live):].any() or live.all()          # the list is a prefix, the padding behind it
            keys = [cols.facet_keys[f] for f in ids[q, r][live]]
            assert all(k[0] == fl.facet_namespace(ns) for k in keys)
            per[ns] = ([(k[1], int(c)) for k, c in zip(keys, counts[q, r][live])], int(distinct[q, r]))
        got.append((int(rows[q]), per))
    return got


def check(cols, rows, names, bits, top, nq=None, stride=None, workspace=None, memo=None):
    """Run one call and compare every query with the oracle; `memo` shares oracle answers between equal masks."""
    torch.cuda.synchronize()
    masks = None if bits is None else pack(bits, stride)
    out = cols.counts(names, masks=masks, nq=nq, top=top, workspace=workspace)
    torch.cuda.synchronize()
    got = answer(cols, names, out)
    memo = {} if memo is None else memo
    for q, g in enumerate(got):
        b = None if bits is None else bits[q]
        key = (top, None if b is None else b.tobytes())
        if key not in memo:
            memo[key] = facet_oracle.facets(rows, b, names, top)
        assert g == memo[key], (q, top)
    return got, out


# ---- 1. row counts at the edges of a group and a span -----------------------------------------------------------
@pytest.mark.parametrize("n,extra", [(0, 0), (1, 0), (63, 0), (64, 0), (65, 0), (1023, 0), (1024, 0), (1025, 0), (2049, 0), (4097, 24)])
def test_row_counts_at_tile_edges(gpu, n, extra):
    rng = np.random.default_rng(n)
    rows = random_rows(rng, n)
    cols = columns(rows)
    bits = np.stack([rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool)])
    stride = fl.mask_bytes(n) + extra
    got, _ = check(cols, rows, NAMES, bits, 10, stride=stride)
    assert [g[0] for g in got] == [int(bits[0].sum()), n, 0]
    unmasked, _ = check(cols, rows, NAMES, None, 10, nq=2)
    assert unmasked[0] == unmasked[1] == got[1]                            # no mask == all ones, junk bits included
    if n >= 63:
        assert got[1][1]["speaker"][1] == 8 and got[1][1]["entity:SERVICE"][1] > 10 and got[1][1]["entity:ABSENT"] == ([], 0)


# ---- 2. batch sizes and masks -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_1025():
    rows = random_rows(np.random.default_rng(1025), 1025)
    return rows, {}


@pytest.mark.parametrize("nq", [1, 2, 31, 32, 33, 64])
def test_batch_sizes_and_masks(gpu, table_1025, nq):
    rows, memo = table_1025
    cols = columns(rows)
    rng = np.random.default_rng(nq)
    bits = mask_set(rng, nq, len(rows))
    got, _ = check(cols, rows, NAMES, bits, 10, memo=memo)
    assert got[0][0] == 0 and all(v == ([], 0) for v in got[0][1].values())             # all zero: all counts zero
    check(cols, rows, NAMES, None, 10, nq=nq, memo=memo)
    check(cols, rows, NAMES, np.ones((nq, len(rows)), bool), 3, memo=memo)
    check(cols, rows, NAMES, np.zeros((nq, len(rows)), bool), 3, memo=memo)


# ---- 3. shapes that break a naive kernel ------------------------------------------------------------------------
def test_a_hot_attribute_and_attributes_that_straddle_a_chunk(gpu):
    # entity:A "hot" on every one of 9000 rows: two whole chunks of 4096 postings are one attribute (the LDS route) and
    # the third is shared; "kind": 4000 + 500 + 4500 postings, so "b" straddles the first chunk edge and "c" two more
    n = 9000
    rows = [[("entity:A", "hot"), ("kind", "a" if i < 4000 else "b" if i < 4500 else "c")] for i in range(n)]
    cols = columns(rows)
    rng = np.random.default_rng(9)
    bits = mask_set(rng, 33, n)
    got, _ = check(cols, rows, ["entity:A", "kind"], bits, 10)
    assert got[1][1] == {"entity:A": ([("hot", n)], 1), "kind": ([("c", 4500), ("a", 4000), ("b", 500)], 3)}
    check(cols, rows, ["kind", "entity:A"], None, 1, nq=64)


def test_the_long_tail_duplicates_and_a_long_row(gpu):
    n = 2049
    rows = [[("entity:T", f"t{i:05d}")] for i in range(n)]                             # every row its own attribute
    rows[5] = [("entity:T", "t00005")] * 5                                             # the same attribute 5 times
    rows[7] = [("entity:T", "t00007")] + [("entity:W", f"w{j:03d}") for j in range(300)]   # a row with 300 attributes
    rows[8] = [("entity:T", "t00008"), ("entity:W", "w001"), ("entity:W", "w001"), ("kind", "k")]
    cols = columns(rows)
    assert cols.n_postings == n + 300 + 2
    rng = np.random.default_rng(4)
    bits = mask_set(rng, 5, n)
    got, _ = check(cols, rows, ["entity:T", "entity:W"], bits, 64)
    assert got[1][1]["entity:T"][1] == n and got[1][1]["entity:T"][0][4:6] == [("t00004", 1), ("t00005", 1)]
    assert got[1][1]["entity:W"] == ([("w001", 2)] + [(f"w{j:03d}", 1) for j in range(64) if j != 1], 300)


def test_only_requested_namespaces_are_counted(gpu):
    rng = np.random.default_rng(12)
    rows = random_rows(rng, 700)
    cols = columns(rows)
    bits = mask_set(rng, 4, 700)
    one, _ = check(cols, rows, ["kind"], bits, 10)
    both, _ = check(cols, rows, ["entity:ABSENT", "kind", "entity:nothing here"], bits, 10)
    assert [g[1]["kind"] for g in one] == [g[1]["kind"] for g in both]
    assert all(g[1]["entity:ABSENT"] == ([], 0) and g[1]["entity:nothing here"] == ([], 0) for g in both)
    none = cols.counts([], masks=pack(bits), top=3)                                     # no namespace: the rows alone
    torch.cuda.synchronize()
    assert tuple(none[0].shape) == (4, 0, 3) and none[3].tolist() == [int(b.sum()) for b in bits]
    assert cols.counts([], nq=2)[3].tolist() == [700, 700]


# ---- 4. selection -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder():
    """1500 values whose counts rise with the value (1 + j // 100): every tile of the selection beats the threshold of
    the one before, so the buffer fills and is sorted again and again; exact ties of 100 values at every count."""
    rows = [[("entity:L", f"v{j:04d}")] for j in reversed(range(1500)) for _ in range(1 + j // 100)]
    return rows, {}


@pytest.mark.parametrize("top", [1, 10, 64])
def test_selection_under_a_rising_threshold(gpu, ladder, top):
    rows, memo = ladder
    cols = columns(rows)
    rng = np.random.default_rng(top)
    bits = np.stack([np.ones(len(rows), bool), rng.random(len(rows)) < 0.5, np.zeros(len(rows), bool)])
    got, _ = check(cols, rows, ["entity:L"], bits, top, memo=memo)
    assert got[0][1]["entity:L"] == ([(f"v{j:04d}", 15) for j in range(1400, 1400 + top)], 1500)   # distinct above top
    assert got[2][1]["entity:L"] == ([], 0)


def test_ties_across_the_cut_go_by_value_whatever_the_dictionary_numbering(gpu):
    values = [f"name {j:02d}" for j in range(30)]
    rows = [[("entity:N", v)] for v in reversed(values)] * 2 + [[("entity:N", "name 17")]]    # first appearance: descending
    attrs = fl.AttributeColumns(rows)
    assert attrs.id_of[("entity:N", "name 29")] == 0 and attrs.id_of[("entity:N", "name 00")] == 29
    cols = fl.FacetColumns(attrs, device=DEV)
    for top in (1, 10, 29):
        got, _ = check(cols, rows, ["entity:N"], None, top)
        want = [("name 17", 3)] + [(v, 2) for v in values if v != "name 17"]
        assert got[0][1]["entity:N"] == (want[:top], 30)


# ---- 5. the query split -----------------------------------------------------------------------------------------
def test_a_small_workspace_splits_the_batch_and_changes_nothing(gpu, table_1025):
    rows, memo = table_1025
    cols = columns(rows)
    bits = mask_set(np.random.default_rng(64), 64, len(rows))
    _, whole = check(cols, rows, NAMES, bits, 10, memo=memo)
    lo, hi = cols.requested(NAMES)
    width = int((hi - lo).sum())
    small = torch.empty(len(rows) * 8 + 5 * width * 4, dtype=torch.uint8, device=DEV)       # five queries at a time
    _, split = check(cols, rows, NAMES, bits, 10, workspace=small, memo=memo)
    for a, b in zip(whole, split):
        assert torch.equal(a, b)
    tiny = torch.empty(len(rows) * 8 + width * 4 - 1, dtype=torch.uint8, device=DEV)         # not even one
    with pytest.raises(ValueError, match="namespace widths"):
        cols.counts(NAMES, masks=pack(bits), top=10, workspace=tiny)
    torch.cuda.synchronize()


# ---- 6. repeatability -------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(gpu):
    rng = np.random.default_rng(8)
    rows = random_rows(rng, 9000)
    cols = columns(rows)
    masks = pack(mask_set(rng, 64, 9000))
    runs = []
    for _ in range(2):
        out = cols.counts(NAMES, masks=masks, top=64)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy().tobytes() for t in out])
    assert runs[0] == runs[1]


# ---- 7. through the table and the retrieve path -----------------------------------------------------------------
DIM = 1024   # the dimension every other suite drives the index at
T0 = datetime(2024, 3, 1, 9, 0, 0)
CALLS = [UUID(int=i + 1) for i in range(9)]
TAGS = {CALLS[0]: ["billing"], CALLS[1]: ["billing", "outage"], CALLS[2]: ["outage"], CALLS[5]: ["renewal"]}
SPEAKERS = ("Alice", "bob", " Carol  Ng ", None)
KINDS = ("summary", "Action Items", "notes")
SERVICES = ("api-gateway", "Billing", "auth", "search")
REQUESTED = ["speaker", "kind", "entity:SERVICE", "entity:ticket", "entity:none"]


def unit(rng, n):
    v = rng.standard_normal((n, DIM)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def table_rows(id_field, ids, body):
    ids = list(ids)
    cols = {id_field: ids, "call_id": [CALLS[(i * 7) % 9] for i in ids], body: [f"timeout shard row {i}" for i in ids],
            "entities": [[("service", SERVICES[i % 4])] * (1 + i % 2) + ([{"label": "Ticket", "value": f"OPS-{i % 13}"}] if i % 3 else [])
                         for i in ids]}
    if id_field == "chunk_id":
        cols.update(speaker=[SPEAKERS[i % 4] for i in ids], start_ts_ms=[i for i in ids], end_ts_ms=[i + 1 for i in ids])
    else:
        cols.update(artifact_id=[i // 2 for i in ids], kind=[KINDS[i % 3] for i in ids])
    return cols, [None if i % 11 == 3 else T0 + timedelta(hours=(i * 5) % 200) for i in ids]


@pytest.fixture()
def world(gpu, monkeypatch):
    rng = np.random.default_rng(77)
    cvec, avec = unit(rng, 340), unit(rng, 120)
    chunks = rt.DenseTable("chunks", "chunk_id", dim=DIM, capacity=400)
    arts = rt.DenseTable("artifact_chunks", "artifact_chunk_id", dim=DIM, capacity=200)
    cols, started = table_rows("chunk_id", range(1000, 1300), "text")
    chunks.add(cvec[:300], cols, call_started_at=started, call_tags=TAGS)
    cols, started = table_rows("artifact_chunk_id", range(500, 620), "content")
    arts.add(avec, cols, call_started_at=started, call_tags=TAGS)
    be = rt.GpuRetrieveBackend(chunks, arts, calls=[{"call_id": c, "external_id": f"ext-{i % 4}", "external_source": "zoom"}
                                                     for i, c in enumerate(CALLS)])
    qvec = (cvec[17] + avec[5]).tolist()
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec for _ in texts], model="m"))
    yield dict(chunks=chunks, arts=arts, be=be, cvec=cvec)
    chunks.close()
    arts.close()


def filter_cases():
    F = rt.RetrieveFilters
    at = T0 + timedelta(hours=55)
    api = {"label": "service", "value": "API-Gateway"}
    return [(None, None), (F(), None), (F(entity_filters=[api]), None), (F(speakers=["ALICE", "carol ng"]), None),
            (F(kinds=["action  items"], date_to=at), CALLS[2:]), (F(date_from=at - timedelta(hours=40)), None),
            (F(entity_filters=[api], call_tags=["outage", "billing"]), None), (F(date_from=at), CALLS[:5]),
            (F(entity_filters=[{"label": "service", "value": "nobody"}]), None), (F(call_tags=["renewal"]), [])]


def host_facets(table, filters, call_ids, names, top):
    rows, per = fl.facets_host(table._row_attrs(), table.filter_mask(filters, call_ids), names, top)
    return {"rows": rows, "facets": {ns: {"values": [{"value": v, "count": c} for v, c in values], "distinct": distinct}
                                     for ns, (values, distinct) in per.items()}}


def assert_facets_follow(table):
    batch = filter_cases()
    got = table.facets(batch, REQUESTED, top=5)
    assert len(got) == len(batch)
    for (filters, call_ids), g in zip(batch, got):
        assert g == host_facets(table, filters, call_ids, REQUESTED, 5), (table.name, filters, call_ids)
    assert table.facets(batch[:2], REQUESTED, top=5) == got[:2]                       # nothing filtered: no mask is built
    return got


def test_table_facets_equal_the_host_rule_and_follow_edits(world):
    chunks, arts, cvec = world["chunks"], world["arts"], world["cvec"]
    got = assert_facets_follow(chunks)
    assert got[0]["rows"] == 300 and got[0]["facets"]["speaker"]["distinct"] == 3 and got[0]["facets"]["kind"]["distinct"] == 0
    assert got[0]["facets"]["entity:SERVICE"]["values"][0] == {"value": "api-gateway", "count": 75}
    assert got[0]["facets"]["entity:ticket"]["distinct"] == 13 and len(got[0]["facets"]["entity:ticket"]["values"]) == 5
    assert 0 < got[2]["rows"] < 300 and got[8]["rows"] == 0 and got[9]["rows"] == 0
    assert assert_facets_follow(arts)[0]["facets"]["speaker"] == {"values": [], "distinct": 0}
    cols = chunks.facet_columns()
    assert cols is chunks.facet_columns() and cols.generation == chunks.generation     # one build per generation
    assert chunks.delete([1003, 1120, 1121]) == 3
    assert_facets_follow(chunks)
    assert chunks.facet_columns() is not cols and chunks.facet_columns().n == len(chunks) == 297
    late, started = table_rows("chunk_id", [1400, 37, 41, 1500], "text")               # ids below the stored ones
    chunks.insert(cvec[300:304], late, call_started_at=started)
    assert assert_facets_follow(chunks)[0]["rows"] == 301
    with pytest.raises(ValueError):
        chunks.facets([(None, None)], ["kind"], top=65)
    with pytest.raises(ValueError):
        chunks.facets([(None, None)] * 65, ["kind"])


def test_the_retrieve_path_equals_the_cpu_composition(world, monkeypatch):
    be = world["be"]
    F = rt.RetrieveFilters
    for filters in (None, F(speakers=["alice", "bob"]), F(entity_filters=[{"label": "service", "value": "auth"}], external_id="ext-1",
                                                          external_source="zoom")):
        for style, query in (("evidence_pack_json", "timeout shard"), ("ids_only", "timeout shard"), ("ids_only", " ")):
            resp = rt.retrieve_evidence(rt.RetrieveRequest(query=query, filters=filters, return_style=style,
                                                           facets=["entity:SERVICE", "speaker", "kind"], facet_top=3), be)
            call_ids = be.resolve_call_ids(filters)
            assert resp["facets"] == {name: host_facets(table, filters, call_ids, ["entity:SERVICE", "speaker", "kind"], 3)
                                      for name, table in be.tables.items()}, (filters, style, query)
            plain = rt.retrieve_evidence(rt.RetrieveRequest(query=query, filters=filters, return_style=style), be)
            for r in (resp, plain):
                r.pop("query_id")
            resp.pop("facets")
            assert resp == plain
    assert resp != {} and plain.get("retrieved_ids") == []


def test_a_request_without_facets_never_builds_the_facet_columns(world, monkeypatch):
    be, chunks, arts = world["be"], world["chunks"], world["arts"]
    built = []
    real_init = fl.FacetColumns.__init__

    def counting_init(self, *a, **k):
        built.append(1)
        real_init(self, *a, **k)

    monkeypatch.setattr(fl.FacetColumns, "__init__", counting_init)
    F = rt.RetrieveFilters
    for filters in (None, F(speakers=["alice"]), F(date_from=T0)):
        for facets in (None, []):
            rt.retrieve_evidence(rt.RetrieveRequest(query="timeout shard", filters=filters, facets=facets), be)
    chunks.filter_masks_device([(F(speakers=["alice"]), None)])
    assert not built and chunks._facet_cols is None and arts._facet_cols is None
    rt.retrieve_evidence(rt.RetrieveRequest(query="timeout shard", facets=["speaker"]), be)   # and with them, once per table
    assert len(built) == 2
