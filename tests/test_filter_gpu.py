"""Filter masks on the GPU: crag_filter_masks_host against the numpy rule (tests/filter_oracle.py), byte for byte
including everything it must leave zero or untouched; DenseTable.filter_mask_device against the host filter_mask
through every lane of GpuRetrieveBackend; filter_masks_device as the per-query masks of HybridSearcher."""
import ctypes
from datetime import datetime, timedelta, timezone
from uuid import UUID

import numpy as np
import pytest
import torch

import filter_oracle
from cadence_rag_amd import embeddings
from cadence_rag_amd import filters as fl
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.dense_index import DenseIndex
from cadence_rag_amd.fusion import HybridSearcher

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 300, 4097, 70001]
NQS = [1, 2, 33, 64]
GUARD = 64
I64_MIN, I64_MAX = filter_oracle.I64_MIN, filter_oracle.I64_MAX


# ---- the kernel against the rule --------------------------------------------------------------------------------
_inputs: dict = {}


def inputs(n):
    """Columns and 64 queries' predicates for a table of n rows, with the rule's answer at the minimal stride --
    computed once per size and shared by every case (fewer queries = the first nq of these)."""
    if n in _inputs:
        return _inputs[n]
    rng = np.random.default_rng(1000 + n)
    n_calls = max(1, min(n // 2, 41))
    ts = rng.integers(0, 500, n).astype(np.int64) * 1_000_000 + 1_700_000_000_000_000
    ts[rng.random(n) < 0.15] = I64_MIN                         # NaT rows
    slot = rng.integers(0, n_calls, n).astype(np.int32)
    if n >= 2:
        slot[n // 2] = -1                                      # rows whose slot lies outside the dictionary
        slot[n - 1] = n_calls
        ts[n - 1] = 1_700_000_000_000_000 + 250_000_000        # (not NaT: only the slot decides)
    kinds = rng.integers(0, 4, 64)                             # no bound / from / to / both
    lo = np.where(kinds & 1, 1_700_000_000_000_000 + rng.integers(0, 300, 64) * 1_000_000, I64_MIN).astype(np.int64)
    hi = np.where(kinds & 2, 1_700_000_000_000_000 + rng.integers(200, 500, 64) * 1_000_000, I64_MAX).astype(np.int64)
    if n:
        real = ts[ts != I64_MIN]
        if real.size:
            lo[1], hi[1] = real[0], real[0]                    # inclusive on both sides: exactly that instant passes
    qset = rng.integers(0, 1 << 63, n_calls, dtype=np.int64).astype(np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n_calls).astype(np.uint64)
    unscoped = np.uint64(sum(1 << q for q in (0, 5, 33, 63)))  # queries without call scoping: their bit in every word
    qset |= unscoped
    held = dict(n=n, n_calls=n_calls, ts=ts, slot=slot, lo=lo, hi=hi, qset=qset,
                d_ts=torch.from_numpy(ts).to(DEV), d_slot=torch.from_numpy(slot).to(DEV))
    held["want"] = filter_oracle.filter_masks(ts, slot, n_calls, qset, lo, hi, fl.mask_bytes(n))
    held["want_unscoped"] = filter_oracle.filter_masks(ts, slot, n_calls, None, lo, hi, fl.mask_bytes(n))
    _inputs[n] = held
    return held


@pytest.fixture(scope="module")
def slot(gpu):
    handle = gpu.crag_upload_slot_create()
    assert handle
    yield handle
    gpu.crag_upload_slot_destroy(handle)


def run(lib, slot, d, qset, lo, hi, nq, stride, buf=None):
    """One call into a 0xAB-filled buffer (or the given one) with 64 guard bytes on both sides: (runs [nq, stride],
    front guard, back guard, the buffer)."""
    if buf is None:
        buf = torch.full((GUARD + nq * stride + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    lo, hi = np.ascontiguousarray(lo[:nq]), np.ascontiguousarray(hi[:nq])
    n = d["n"]
    rc = lib.crag_filter_masks_host(d["d_ts"].data_ptr() if n else None, d["d_slot"].data_ptr() if n else None, n,
                                    d["n_calls"], None if qset is None else qset.ctypes.data, lo.ctypes.data,
                                    hi.ctypes.data, nq, slot, buf.data_ptr() + GUARD, stride,
                                    ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, lib.crag_last_error()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + nq * stride].reshape(nq, stride), host[:GUARD], host[GUARD + nq * stride:], buf


def padded(want, nq, stride):
    out = np.zeros((nq, stride), dtype=np.uint8)
    out[:, :want.shape[1]] = want[:nq]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_rule_at_every_stride(gpu, slot, n):
    d = inputs(n)
    for nq in NQS:
        for extra in (0, 4, 64):
            stride = fl.mask_bytes(n) + extra
            got, front, back, _ = run(gpu, slot, d, d["qset"], d["lo"], d["hi"], nq, stride)
            assert np.array_equal(got, padded(d["want"], nq, stride)), (n, nq, stride)
            assert np.all(front == 0xAB) and np.all(back == 0xAB), (n, nq, stride)


@pytest.mark.parametrize("n", [97, 1025])
def test_kernel_at_the_half_boundary_of_the_transpose(gpu, slot, n):
    """nq around 32, where the ballot transpose goes from the low half of a row's query set to the high one, and 63, one
    short of a full wave.  97 rows: one full and one partial group; 1025 rows: one full span plus one row, and at the
    minimal stride the words behind that row's belong to the next query's run."""
    d = inputs(n)
    for nq in (31, 32, 63):
        for extra in (0, 4):
            stride = fl.mask_bytes(n) + extra
            got, front, back, _ = run(gpu, slot, d, d["qset"], d["lo"], d["hi"], nq, stride)
            assert np.array_equal(got, padded(d["want"], nq, stride)), (n, nq, stride)
            assert np.all(front == 0xAB) and np.all(back == 0xAB), (n, nq, stride)


@pytest.mark.parametrize("n", [1, 33, 97, 4097])
def test_kernel_without_a_call_table_and_without_any_filter(gpu, slot, n):
    d = inputs(n)
    stride = fl.mask_bytes(n) + 4
    for nq in NQS:
        got, front, back, _ = run(gpu, slot, d, None, d["lo"], d["hi"], nq, stride)
        assert np.array_equal(got, padded(d["want_unscoped"], nq, stride)), (n, nq)
        assert np.all(front == 0xAB) and np.all(back == 0xAB)
        open_lo, open_hi = np.full(64, I64_MIN, dtype=np.int64), np.full(64, I64_MAX, dtype=np.int64)
        got, _, _, _ = run(gpu, slot, d, None, open_lo, open_hi, nq, stride)
        ones = padded(DenseIndex.pack_mask(np.ones((nq, n), dtype=bool)), nq, stride)    # NaT rows included
        assert np.array_equal(got, ones), (n, nq)


def test_rows_outside_the_call_table_and_nat_rows(gpu, slot):
    """The rows with slot -1 and slot n_calls pass no query when a call table is given -- not even an unscoped one's
    all-ones column, which lives in the table -- and every query when none is; a NaT row passes exactly the queries
    without a date bound."""
    d = inputs(300)
    got, _, _, _ = run(gpu, slot, d, d["qset"], d["lo"], d["hi"], 64, fl.mask_bytes(300))
    bit = lambda q, i: (got[q, i >> 3] >> (i & 7)) & 1
    for i in (150, 299):
        assert d["slot"][i] in (-1, d["n_calls"]) and not any(bit(q, i) for q in range(64))
    nat = [i for i in np.flatnonzero(d["ts"] == I64_MIN) if 0 <= d["slot"][i] < d["n_calls"]][:5]
    assert nat
    for i in nat:
        for q in (0, 5, 33, 63):   # unscoped queries
            dated = d["lo"][q] != I64_MIN or d["hi"][q] != I64_MAX
            assert bit(q, i) == (0 if dated else 1), (q, i)


def test_a_reused_buffer_keeps_no_stale_bit(gpu, slot):
    d = inputs(4097)
    stride = fl.mask_bytes(4097) + 4
    _, _, _, buf = run(gpu, slot, d, None, np.full(64, I64_MIN, dtype=np.int64), np.full(64, I64_MAX, dtype=np.int64),
                       64, stride)                                                   # all ones first
    got, front, back, _ = run(gpu, slot, d, d["qset"], d["lo"], d["hi"], 64, stride, buf=buf)
    assert np.array_equal(got, padded(d["want"], 64, stride))
    assert np.all(front == 0xAB) and np.all(back == 0xAB)


# ---- through the table ------------------------------------------------------------------------------------------
DIM = 1024   # the dimension every other suite drives the index at
T0 = datetime(2024, 3, 1, 9, 0, 0)
CALLS = [UUID(int=i + 1) for i in range(9)]
TAGS = {CALLS[0]: ["billing"], CALLS[1]: ["billing", "outage"], CALLS[2]: ["outage"], CALLS[3]: [], CALLS[4]: None,
        CALLS[5]: ["renewal"], CALLS[6]: ["outage", "renewal"]}          # calls 7 and 8 are absent
WORDS = ("timeout", "retry", "invoice", "shard", "latency", "refund", "login", "export")


def unit(rng, n):
    v = rng.standard_normal((n, DIM)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def table_rows(id_field, ids, body):
    ids = list(ids)
    cols = {id_field: ids, "call_id": [CALLS[(i * 7) % 9] for i in ids],
            body: [f"{WORDS[i % 8]} {WORDS[(i // 3) % 8]} row {i}" for i in ids],
            "tech_tokens": [["ECONNRESET"] if i % 4 == 0 else [f"TOK-{i % 5}"] for i in ids]}
    if id_field == "chunk_id":
        cols.update(speaker=["S"] * len(ids), start_ts_ms=[i for i in ids], end_ts_ms=[i + 1 for i in ids])
    else:
        cols.update(artifact_id=[i // 2 for i in ids], kind=["summary"] * len(ids))
    started = [None if i % 11 == 3 else T0 + timedelta(hours=(i * 5) % 200) for i in ids]
    return cols, started


@pytest.fixture()
def world(gpu, monkeypatch):
    rng = np.random.default_rng(77)
    cvec, avec = unit(rng, 340), unit(rng, 120)
    chunks = rt.DenseTable("chunks", "chunk_id", dim=DIM, capacity=400)
    arts = rt.DenseTable("artifact_chunks", "artifact_chunk_id", dim=DIM, capacity=200)
    cols, started = table_rows("chunk_id", range(1000, 1300), "text")
    ctok = cols.pop("tech_tokens")
    chunks.add(cvec[:300], cols, call_started_at=started, call_tags=TAGS)
    cols, started = table_rows("artifact_chunk_id", range(500, 620), "content")
    atok = cols.pop("tech_tokens")
    arts.add(avec, cols, call_started_at=started, call_tags=TAGS)
    be = rt.GpuRetrieveBackend(chunks, arts, calls=[{"call_id": c, "external_id": f"ext-{i % 4}", "external_source": "zoom"}
                                                     for i, c in enumerate(CALLS)],
                               bm25_chunks=chunks.build_bm25_lane("text"), bm25_artifacts=arts.build_bm25_lane("content"),
                               tech_chunks=chunks.build_tech_lane(ctok), tech_artifacts=arts.build_tech_lane(atok))
    qvec = (cvec[17] + avec[5]).tolist()
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec for _ in texts], model="m"))
    yield dict(chunks=chunks, arts=arts, be=be, cvec=cvec, qvec=qvec)
    chunks.close()
    arts.close()


def filter_cases():
    F = rt.RetrieveFilters
    at = T0 + timedelta(hours=55)        # the timestamp of rows with (5 i) % 200 == 55: inclusive bounds
    aware = at.replace(tzinfo=timezone.utc).astimezone(timezone(timedelta(hours=-8)))
    return [(None, None), (F(), None), (None, CALLS[:2]), (F(date_from=at), None), (F(date_to=at), None),
            (F(date_from=at - timedelta(hours=40), date_to=aware), None), (F(), []), (F(), CALLS[2:5]),
            (F(), [UUID(int=99)]), (F(call_tags=["outage"]), None), (F(call_tags=["nope"]), None),
            (F(call_tags=["outage", "billing"]), CALLS[1:4]), (F(date_from=at - timedelta(hours=60), call_tags=["renewal"]), CALLS[4:])]


def host_route(table, filters, call_ids):
    """What every caller did before the device route existed: the host mask, packed and uploaded."""
    mask = rt.DenseTable.filter_mask(table, filters, call_ids)
    return None if mask is None else torch.from_numpy(DenseIndex.pack_mask(mask)).to(DEV)


def assert_masks_follow(table):
    for filters, call_ids in filter_cases():
        got, want = table.filter_mask_device(filters, call_ids), table.filter_mask(filters, call_ids)
        if want is None:
            assert got is None, (filters, call_ids)
        else:
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (fl.mask_bytes(len(table)),)
            assert np.array_equal(got.cpu().numpy(), DenseIndex.pack_mask(want)), (filters, call_ids)


def test_table_masks_equal_the_host_masks_and_follow_edits(world):
    chunks, cvec = world["chunks"], world["cvec"]
    assert_masks_follow(chunks)
    assert_masks_follow(world["arts"])
    cols = chunks.filter_columns()
    assert cols is chunks.filter_columns() and cols.generation == chunks.generation     # one build per generation
    f = rt.RetrieveFilters(call_tags=["outage"])
    assert chunks.filter_mask_device(f, CALLS[:3]) is chunks.filter_mask_device(f, CALLS[:3])   # one mask per request
    assert chunks.delete_calls([CALLS[2], CALLS[7]]) > 0
    assert_masks_follow(chunks)
    assert chunks.filter_columns() is not cols and chunks.filter_columns().n == len(chunks)
    late, started = table_rows("chunk_id", [1400, 37, 41, 1500], "text")                # ids below the stored ones
    chunks.insert(cvec[300:304], late, call_started_at=started)
    assert_masks_follow(chunks)
    batch = filter_cases()
    masks, stride = chunks.filter_masks_device(batch)
    assert stride == fl.mask_bytes(len(chunks)) and tuple(masks.shape) == (len(batch), stride)
    for q, (filters, call_ids) in enumerate(batch):
        want = chunks.filter_mask(filters, call_ids)
        want = np.ones(len(chunks), dtype=bool) if want is None else want
        assert np.array_equal(masks[q].cpu().numpy(), DenseIndex.pack_mask(want)), q
    with pytest.raises(ValueError):
        chunks.filter_masks_device([(None, None)] * 65)


def lane_answers(be, qvec, filters):
    call_ids = be.resolve_call_ids(filters)
    return (be.estimate_dense_candidates("chunks", filters, call_ids), be.estimate_dense_candidates("artifact_chunks", filters, call_ids),
            be.fetch_chunks_dense(qvec, filters, call_ids, "exact", 50), be.fetch_artifacts_dense(qvec, filters, call_ids, "exact", 10),
            be.fetch_chunks_bm25("timeout shard row", filters, call_ids, 50), be.fetch_artifacts_bm25("refund latency", filters, call_ids, 10),
            be.fetch_chunks_tech(["ECONNRESET", "TOK-2"], filters, call_ids, 50), be.fetch_artifacts_tech(["ECONNRESET"], filters, call_ids, 50))


def response(be, filters):
    resp = rt.retrieve_evidence(rt.RetrieveRequest(query="timeout shard ECONNRESET refund", filters=filters, debug=True,
                                                   budget=rt.Budget(max_evidence_items=12, max_total_chars=20000)), be)
    resp.pop("query_id")
    return resp


def request_filters():
    F = rt.RetrieveFilters
    at = T0 + timedelta(hours=55)
    return [None, F(date_from=at), F(date_from=at - timedelta(hours=50), date_to=at + timedelta(hours=20)),
            F(call_ids=CALLS[:4]), F(external_id="ext-1", external_source="zoom"), F(call_tags=["outage"]),
            F(call_ids=CALLS[1:6], call_tags=["outage", "renewal"], date_to=at + timedelta(hours=90)),
            F(external_id="nobody")]


def test_every_lane_and_the_response_match_the_host_route(world, monkeypatch):
    be, qvec = world["be"], world["qvec"]
    got = [(lane_answers(be, qvec, f), response(be, f)) for f in request_filters()]
    monkeypatch.setattr(rt.DenseTable, "filter_mask_device", host_route)
    want = [(lane_answers(be, qvec, f), response(be, f)) for f in request_filters()]
    for f, g, w in zip(request_filters(), got, want):
        assert g == w, f
    scoped = got[3]
    assert 0 < scoped[0][0] < len(world["chunks"]) and scoped[0][2] and scoped[0][4] and scoped[0][6]
    assert scoped[1]["quotes"] and all(UUID(q["call_id"]) in CALLS[:4] for q in scoped[1]["quotes"])


def test_a_scoped_request_never_walks_the_rows_on_the_host(world, monkeypatch):
    def walked(self, filters, call_ids):
        raise AssertionError("the host filter_mask ran inside a request")

    monkeypatch.setattr(rt.DenseTable, "filter_mask", walked)
    f = rt.RetrieveFilters(call_ids=CALLS[:4], call_tags=["outage", "billing"], date_from=T0 + timedelta(hours=5))
    resp = response(world["be"], f)
    assert resp["quotes"] and {UUID(q["call_id"]) for q in resp["quotes"]} <= {CALLS[0], CALLS[1], CALLS[2]}
    assert resp["notes"]["retrieval"]["dense_candidate_rows"]["chunks"] > 0


# ---- batch ------------------------------------------------------------------------------------------------------
def test_hybrid_search_takes_the_per_query_device_masks(world):
    chunks, be = world["chunks"], world["be"]
    rng = np.random.default_rng(5)
    pool = filter_cases()
    batch = [pool[q % len(pool)] for q in range(64)]
    queries = torch.from_numpy(unit(rng, 64)).to(DEV)
    tokens = [["ECONNRESET"] if q % 2 else [f"TOK-{q % 5}", "ECONNRESET"] for q in range(64)]
    texts = [f"{WORDS[q % 8]} {WORDS[(q + 3) % 8]} row" for q in range(64)]
    searcher = HybridSearcher(chunks.index, be._tech["chunks"], dense_k=20, tech_k=20, bm25_index=be._bm25["chunks"], bm25_k=20)
    keys = ("ids", "counts", "dense_ids", "dense_counts", "bm25_ids", "bm25_counts")

    def step(mask, stride):
        out = searcher.search(queries, tokens, query_texts=texts, row_mask=mask, mask_stride=stride)
        torch.cuda.synchronize()
        return {k: out[k].cpu().numpy().copy() for k in keys}

    d_masks, stride = chunks.filter_masks_device(batch)
    got = step(d_masks, stride)
    host = np.stack([np.ones(len(chunks), dtype=bool) if (m := chunks.filter_mask(f, c)) is None else m for f, c in batch])
    packed = DenseIndex.pack_mask(host)
    assert packed.shape == (64, stride)
    want = step(torch.from_numpy(packed).to(DEV), stride)
    for k in keys:
        assert np.array_equal(got[k], want[k]), k
    assert got["counts"].max() > 0 and got["counts"][6] == 0        # (F(), []) admits nothing
