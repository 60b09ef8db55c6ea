"""Attribute masks on the GPU: crag_attr_masks_host against the rule (tests/attr_oracle.py), byte for byte including
everything it must leave zero or untouched -- no tolerance anywhere; the limits of its key table; DenseTable's
filter_mask_device with entity, speaker and kind clauses against the host filter_mask through every lane of
GpuRetrieveBackend; filter_masks_device as the per-query masks of HybridSearcher."""
import ctypes
from datetime import datetime, timedelta
from uuid import UUID

import numpy as np
import pytest
import torch

import attr_oracle
from cadence_rag_amd import _native, embeddings
from cadence_rag_amd import filters as fl
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.dense_index import DenseIndex
from cadence_rag_amd.fusion import HybridSearcher

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049, 70001]
NQS = [1, 2, 33, 64]
HALF_NQS = [31, 32, 63]   # around the 32-bit halves of the ballot transpose, and one short of a full wave
GUARD = 64
N_ATTRS = 300
LISTED = 290          # queries list keys below this; the ids [LISTED, N_ATTRS) are in the dictionary and in no query


@pytest.fixture(scope="module")
def slot(gpu):
    handle = gpu.crag_upload_slot_create()
    assert handle
    yield handle
    gpu.crag_upload_slot_destroy(handle)


# ---- inputs -----------------------------------------------------------------------------------------------------
def skewed(rng, size):
    """Ids below LISTED, half of them from a hot dozen: rows and queries meet often enough for masks of every density."""
    hot = rng.random(size) < 0.5
    return np.where(hot, rng.integers(0, 12, size), rng.integers(0, LISTED, size))


def make_queries(rng):
    """64 queries: 0-8 clauses of 1-5 keys, with the fixed ones the kernel must get right."""
    queries = [[[int(k) for k in skewed(rng, int(rng.integers(1, 6)))] for _ in range(int(rng.integers(0, 9)))]
               for _ in range(64)]
    a, b = [3, 7, 200], [5, 250]
    queries[0] = []                                          # no clauses: every admitted row passes
    queries[1] = [[2, 4], []]                                # a clause without a key: nothing passes
    queries[2] = [[6], [6, 9]]                               # one key in two clauses
    queries[3] = [a, b]                                      # key sets shared across queries ...
    queries[4] = [b, [1, 2, 3], a]                           # ... at other clause numbers
    queries[5] = [[int(k) for k in rng.integers(0, 12, 4)] for _ in range(8)]   # all 8 clauses
    queries[33] = [[0]]
    queries[63] = [a, [0, 1, 2, 3, 4]]
    return queries


_queries: dict = {}


def shared_queries():
    if not _queries:
        q = make_queries(np.random.default_rng(4242))
        _queries.update(lists=q, compiled={nq: attr_oracle.transpose(q[:nq]) for nq in NQS + HALF_NQS})
    return _queries


_inputs: dict = {}


def inputs(n):
    """A CSR of n rows and the rule's answer for the 64 queries at the minimal stride, computed once per size and shared
    by every case (fewer queries = the first nq of these; an input mask is ANDed onto the answer)."""
    if n in _inputs:
        return _inputs[n]
    rng = np.random.default_rng(2000 + n)
    counts = rng.integers(1, 7, n)
    counts[rng.random(n) < 0.15] = 0                          # rows without attributes
    rows = [skewed(rng, int(c)) for c in counts]
    for i in range(0, n, 5):                                  # duplicates inside rows
        if rows[i].size >= 2:
            rows[i][-1] = rows[i][0]
    if n >= 64:
        rows[n // 3] = skewed(rng, 700)                       # one long row
        rows[n // 2] = rng.integers(LISTED, N_ATTRS, 4)       # one row of ids no query lists
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    ids = (np.concatenate(rows) if n and ptr[-1] else np.empty(0)).astype(np.int32)
    q = shared_queries()
    keys, key_sets, clause_sets = q["compiled"][64]
    held = dict(n=n, ptr=ptr, ids=ids, n_attrs=N_ATTRS, d_ptr=torch.from_numpy(ptr).to(DEV),
                d_ids=torch.from_numpy(ids if ids.size else np.zeros(1, dtype=np.int32)).to(DEV))
    held["want"] = attr_oracle.attr_masks(ptr, ids, N_ATTRS, keys, key_sets, clause_sets, 64, fl.mask_bytes(n))
    # input masks, garbage beyond n included: one shared run, and one run per query at a stride of its own
    held["in_shared"] = rng.integers(0, 256, fl.mask_bytes(n) + 4, dtype=np.uint8)
    held["in_per"] = rng.integers(0, 256, (64, fl.mask_bytes(n) + 8), dtype=np.uint8)
    held["d_in_shared"] = torch.from_numpy(held["in_shared"]).to(DEV)
    held["d_in_per"] = torch.from_numpy(held["in_per"]).to(DEV)
    _inputs[n] = held
    return held


def raw_call(lib, slot, d, compiled, nq, out_ptr, stride, in_ptr=None, in_stride=0):
    keys, key_sets, clause_sets = compiled
    keys, key_sets = np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(key_sets, dtype=np.uint64)
    clause_sets = np.ascontiguousarray(clause_sets, dtype=np.uint64)
    n = d["n"]
    return lib.crag_attr_masks_host(d["d_ptr"].data_ptr() if n else None, d["d_ids"].data_ptr() if n else None, n,
                                    d["n_attrs"], keys.ctypes.data if keys.size else None,
                                    key_sets.ctypes.data if keys.size else None, int(keys.size), clause_sets.ctypes.data, nq,
                                    in_ptr, in_stride, slot, out_ptr, stride,
                                    ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def run(lib, slot, d, compiled, nq, stride, in_ptr=None, in_stride=0, buf=None, in_place=None):
    """One call into a 0xAB-filled buffer (or the given one) with 64 guard bytes on both sides: (runs [nq, stride],
    front guard, back guard, the buffer).  in_place: a uint8 [nq, stride] array the runs hold before the call, which
    then reads them as its input mask."""
    if buf is None:
        buf = torch.full((GUARD + nq * stride + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    if in_place is not None:
        buf[GUARD:GUARD + nq * stride] = torch.from_numpy(np.ascontiguousarray(in_place).reshape(-1)).to(DEV)
        in_ptr, in_stride = buf.data_ptr() + GUARD, stride
    rc = raw_call(lib, slot, d, compiled, nq, buf.data_ptr() + GUARD, stride, in_ptr, in_stride)
    assert rc == 0, lib.crag_last_error()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + nq * stride].reshape(nq, stride), host[:GUARD], host[GUARD + nq * stride:], buf


def padded(want, nq, stride):
    out = np.zeros((nq, stride), dtype=np.uint8)
    out[:, :want.shape[1]] = want[:nq]
    return out


def untouched(front, back):
    return bool(np.all(front == 0xAB) and np.all(back == 0xAB))


# ---- 1. the kernel against the rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_rule_at_every_stride_and_input_mask(gpu, slot, n):
    d = inputs(n)
    mb = fl.mask_bytes(n)
    rng = np.random.default_rng(n)
    for nq in NQS:
        compiled = shared_queries()["compiled"][nq]
        for extra in (0, 4, 64):
            stride = mb + extra
            want = padded(d["want"], nq, stride)
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride)                              # no input mask
            assert np.array_equal(got, want) and untouched(front, back), (n, nq, stride, "null")
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride, d["d_in_shared"].data_ptr(), 0)
            assert np.array_equal(got, want & padded(d["in_shared"][None, :mb].repeat(nq, 0), nq, stride)) \
                and untouched(front, back), (n, nq, stride, "shared")
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride, d["d_in_per"].data_ptr(), mb + 8)
            assert np.array_equal(got, want & padded(d["in_per"][:, :mb], nq, stride)) and untouched(front, back), \
                (n, nq, stride, "per query")
            before = rng.integers(0, 256, (nq, stride), dtype=np.uint8)                                # in place
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride, in_place=before)
            assert np.array_equal(got, want & before) and untouched(front, back), (n, nq, stride, "in place")


@pytest.mark.parametrize("n", [97, 1025])
def test_kernel_at_the_half_boundary_of_the_transpose(gpu, slot, n):
    """nq around 32 and at 63, without an input mask, with one run per query and in place.  97 rows: one full and one
    partial group; 1025 rows: one full span plus one row, and at the minimal stride the words behind that row's belong
    to the next query's run."""
    d = inputs(n)
    mb = fl.mask_bytes(n)
    rng = np.random.default_rng(n)
    for nq in HALF_NQS:
        compiled = shared_queries()["compiled"][nq]
        for extra in (0, 4):
            stride = mb + extra
            want = padded(d["want"], nq, stride)
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride)
            assert np.array_equal(got, want) and untouched(front, back), (n, nq, stride, "null")
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride, d["d_in_per"].data_ptr(), mb + 8)
            assert np.array_equal(got, want & padded(d["in_per"][:, :mb], nq, stride)) and untouched(front, back), \
                (n, nq, stride, "per query")
            before = rng.integers(0, 256, (nq, stride), dtype=np.uint8)
            got, front, back, _ = run(gpu, slot, d, compiled, nq, stride, in_place=before)
            assert np.array_equal(got, want & before) and untouched(front, back), (n, nq, stride, "in place")


def test_the_inputs_exercise_the_rule():
    """The shared answer is neither empty nor full, the fixed queries do what they were built for, and the input-mask
    form of the oracle is the AND the cases above apply."""
    d = inputs(2049)
    want, n = d["want"], 2049
    bits = np.unpackbits(want, axis=1, bitorder="little")[:, :n]
    assert bits[0].all() and not bits[1].any()
    assert 0 < bits[2].sum() < n and 0 < bits[3].sum() < n and 0 < bits[63].sum() < n
    open_queries = sum(1 for clauses in shared_queries()["lists"] if not clauses)
    assert bits[:, n // 3].sum() > 20 and bits[:, n // 2].sum() == open_queries    # the long row; the row of unlisted ids
    assert (bits[4] <= bits[3]).all()                                              # query 4 holds query 3's clauses
    keys, key_sets, clause_sets = shared_queries()["compiled"][64]
    mb = fl.mask_bytes(n)
    with_in = attr_oracle.attr_masks(d["ptr"], d["ids"], N_ATTRS, keys, key_sets, clause_sets, 64, mb, d["in_per"], mb + 8)
    assert np.array_equal(with_in, want & d["in_per"][:, :mb])


# ---- 2. the limits of the key table -----------------------------------------------------------------------------
def one_per_row(n, n_attrs, ids):
    ids = np.asarray(ids, dtype=np.int32)
    ptr = np.arange(n + 1, dtype=np.int64)
    return dict(n=n, ptr=ptr, ids=ids, n_attrs=n_attrs, d_ptr=torch.from_numpy(ptr).to(DEV), d_ids=torch.from_numpy(ids).to(DEV))


def keyed_queries(keys, rng):
    """64 queries whose clauses together list exactly `keys`; the even ones hold one clause (a row of one attribute can
    pass them), the odd ones grow more."""
    queries = [[] for _ in range(64)]
    for j, k in enumerate(keys):
        q = j % 64
        if not queries[q] or (q % 2 and len(queries[q]) < 8 and rng.random() < 0.3):
            queries[q].append([])
        queries[q][int(rng.integers(0, len(queries[q])))].append(int(k))
    return queries


@pytest.mark.parametrize("spread", ["consecutive", "multiples of 1024"])
def test_a_full_key_table(gpu, slot, spread):
    """Exactly 512 keys -- as 512 consecutive ids, keys 0 and n_attrs - 1 among them, and as ids that are all multiples
    of 1 024 (long probe chains under any power-of-two table) --, one attribute per row over 4 097 rows."""
    rng = np.random.default_rng(7)
    n = 4097
    if spread == "consecutive":
        n_attrs = 512
        keys = np.arange(512)
        assert keys[0] == 0 and keys[-1] == n_attrs - 1
    else:
        n_attrs = 1 << 20
        keys = np.arange(512) * 1024
    assert keys.size == 512
    near = np.clip(keys[rng.integers(0, 512, n)] + rng.integers(-1, 2, n), 0, n_attrs - 1)   # keys and their neighbours
    ids = np.where(rng.random(n) < 0.7, keys[rng.integers(0, 512, n)], near)
    ids[:2] = (0, n_attrs - 1)
    d = one_per_row(n, n_attrs, ids)
    compiled = attr_oracle.transpose(keyed_queries(keys, rng))
    assert compiled[0].size == 512
    stride = fl.mask_bytes(n)
    want = attr_oracle.attr_masks(d["ptr"], d["ids"], n_attrs, *compiled, 64, stride)
    assert want.any()
    got, front, back, _ = run(gpu, slot, d, compiled, 64, stride)
    assert np.array_equal(got, want) and untouched(front, back)


def test_513_keys_are_too_big_and_the_columns_split_the_batch(gpu, slot):
    rng = np.random.default_rng(8)
    n, n_attrs = 4097, 600
    keys = np.arange(40, 553)
    d = one_per_row(n, n_attrs, rng.integers(0, n_attrs, n))
    queries = keyed_queries(keys, rng)
    compiled = attr_oracle.transpose(queries)
    assert compiled[0].size == 513
    stride = fl.mask_bytes(n)
    buf = torch.full((GUARD + 64 * stride + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    assert raw_call(gpu, slot, d, compiled, 64, buf.data_ptr() + GUARD, stride) == _native.CRAG_E2BIG
    assert b"attr_masks_host" in gpu.crag_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all())                                          # nothing was enqueued
    # AttributeColumns.masks splits the batch by queries: same dictionary ids, rows of one attribute each
    names = [("entity:X", str(i)) for i in range(n_attrs)]
    cols = fl.AttributeColumns([[names[0]]] + [[names[i]] for i in range(1, n_attrs)] + [[names[int(i)]] for i in d["ids"]], device=DEV)
    assert cols.n == n_attrs + n and all(cols.id_of[names[i]] == i for i in range(n_attrs))
    want = attr_oracle.attr_masks(cols.attr_ptr, cols.attr_ids, n_attrs, *compiled, 64, fl.mask_bytes(cols.n))
    got = cols.masks(compiled, nq=64)
    assert tuple(got.shape) == (64, fl.mask_bytes(cols.n)) and np.array_equal(got.cpu().numpy(), want)
    in_mask = torch.from_numpy(rng.integers(0, 256, got.shape, dtype=np.uint8)).to(DEV)
    before = in_mask.cpu().numpy().copy()
    cols.masks(compiled, in_mask=in_mask, in_stride=int(got.shape[1]), out=in_mask)      # split AND in place
    assert np.array_equal(in_mask.cpu().numpy(), want & before)
    one = ([k for k in range(513)], np.zeros((513, 8), dtype=np.uint64), np.asarray([1] + [0] * 7, dtype=np.uint64))
    one[1][:, 0] = 1
    with pytest.raises(ValueError, match="512"):
        cols.masks(one, nq=1)
    cols.close()


# ---- 3. ids outside the dictionary ------------------------------------------------------------------------------
def test_row_ids_outside_the_dictionary_match_nothing(gpu, slot):
    n_attrs = 50
    rows = [[-1], [n_attrs], [2 ** 31 - 1], [49], [0], [-1, 49], [n_attrs, 2 ** 31 - 1, -(2 ** 31)], [0, -1]]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids = np.asarray([a for r in rows for a in r], dtype=np.int32)
    d = dict(n=len(rows), ptr=ptr, ids=ids, n_attrs=n_attrs, d_ptr=torch.from_numpy(ptr).to(DEV), d_ids=torch.from_numpy(ids).to(DEV))
    compiled = attr_oracle.transpose([[[0, 49]], [[49]], [[0], [49]]])
    got, front, back, _ = run(gpu, slot, d, compiled, 3, 4)
    assert got[:, 0].tolist() == [0b10111000, 0b00101000, 0] and not got[:, 1:].any() and untouched(front, back)
    assert np.array_equal(got, attr_oracle.attr_masks(ptr, ids, n_attrs, *compiled, 3, 4))


# ---- 4., 5. reuse and repeatability -----------------------------------------------------------------------------
def test_a_reused_buffer_keeps_no_stale_bit_and_calls_repeat(gpu, slot):
    d = inputs(2049)
    stride = fl.mask_bytes(2049) + 4
    ones_heavy = attr_oracle.transpose([[] if q % 2 else [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]] for q in range(64)])
    got, _, _, buf = run(gpu, slot, d, ones_heavy, 64, stride)
    assert np.unpackbits(got[1]).sum() == 2049 and np.unpackbits(got).sum() > 64 * 2049 // 2
    compiled = shared_queries()["compiled"][64]
    got, front, back, buf = run(gpu, slot, d, compiled, 64, stride, buf=buf)          # a sparse result over it
    assert np.array_equal(got, padded(d["want"], 64, stride)) and untouched(front, back)
    again, _, _, _ = run(gpu, slot, d, compiled, 64, stride)                           # an identical call, a fresh buffer
    assert np.array_equal(again, got)


# ---- 6. argument errors leave the buffer alone ------------------------------------------------------------------
def test_argument_errors_leave_the_buffer_untouched(gpu, slot):
    d = inputs(65)
    keys, key_sets, clause_sets = (x.copy() for x in attr_oracle.transpose([[[1, 5], [9]], [[5]]]))
    stride = fl.mask_bytes(65)
    buf = torch.full((GUARD + 64 * 16 + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf.data_ptr() + GUARD
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(ptr=d["d_ptr"].data_ptr(), ids=d["d_ids"].data_ptr(), n_rows=65, n_attrs=N_ATTRS, keys=keys, key_sets=key_sets,
             n_keys=3, clause_sets=clause_sets, nq=2, in_mask=None, in_stride=0, slot=slot, out=out, stride=stride):
        k = None if keys is None else np.ascontiguousarray(keys, dtype=np.int32)
        s = None if key_sets is None else np.ascontiguousarray(key_sets, dtype=np.uint64)
        c = None if clause_sets is None else np.ascontiguousarray(clause_sets, dtype=np.uint64)
        return gpu.crag_attr_masks_host(ptr, ids, n_rows, n_attrs, None if k is None else k.ctypes.data,
                                        None if s is None else s.ctypes.data, n_keys, None if c is None else c.ctypes.data, nq,
                                        in_mask, in_stride, slot, out, stride, stream)

    not_subset, high_bit, high_key_bit = key_sets.copy(), clause_sets.copy(), key_sets.copy()
    not_subset[0, 1] |= np.uint64(0b10)              # query 1 has no clause 1
    high_bit[0] |= np.uint64(0b100)                  # a bit at nq
    high_key_bit[2, 1] |= np.uint64(1 << 40)
    bad = [dict(nq=0), dict(nq=65), dict(n_rows=-1), dict(n_rows=1 << 31), dict(n_attrs=-1), dict(n_keys=-1),
           dict(keys=[1, 1, 9]), dict(keys=[5, 1, 9]), dict(keys=[-1, 5, 9]), dict(keys=[1, 5, N_ATTRS]),
           dict(clause_sets=high_bit), dict(key_sets=high_key_bit), dict(key_sets=not_subset),
           dict(stride=stride - 4), dict(stride=stride + 2), dict(stride=-4), dict(stride=0),
           dict(in_mask=out, in_stride=stride - 4), dict(in_mask=out, in_stride=stride + 2), dict(in_mask=out + 2),
           dict(out=out + 1), dict(out=out + 2),
           dict(ptr=None), dict(ids=None), dict(keys=None), dict(key_sets=None), dict(clause_sets=None), dict(slot=None),
           dict(out=None)]
    for kw in bad:
        assert call(**kw) == -1, kw            # CRAG_EINVAL
        assert b"attr_masks_host" in gpu.crag_last_error(), kw
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all())
    assert call() == 0                               # and the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xAB).all()) and bool((buf[GUARD + 2 * stride:] == 0xAB).all())


# ---- 7. through the table ---------------------------------------------------------------------------------------
DIM = 1024   # the dimension every other suite drives the index at
T0 = datetime(2024, 3, 1, 9, 0, 0)
CALLS = [UUID(int=i + 1) for i in range(9)]
TAGS = {CALLS[0]: ["billing"], CALLS[1]: ["billing", "outage"], CALLS[2]: ["outage"], CALLS[3]: [], CALLS[5]: ["renewal"],
        CALLS[6]: ["outage", "renewal"]}
WORDS = ("timeout", "retry", "invoice", "shard", "latency", "refund", "login", "export")
SPEAKERS = ("Alice", "bob", " Carol  Ng ", None)
KINDS = ("summary", "Action Items", "notes")
ORGS = ("Acme", "Initech", "Globex")


def unit(rng, n):
    v = rng.standard_normal((n, DIM)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def entities_of(i):
    ents = [("org", ORGS[i % 3])] if i % 4 else []
    if i % 5 == 0:
        ents.append({"label": "Person", "value": "Ada  Lovelace"})
    if i % 7 == 0:
        ents.append(("product", ORGS[(i // 7) % 3]))           # the same value under another label
    return ents


def table_rows(id_field, ids, body):
    ids = list(ids)
    cols = {id_field: ids, "call_id": [CALLS[(i * 7) % 9] for i in ids],
            body: [f"{WORDS[i % 8]} {WORDS[(i // 3) % 8]} row {i}" for i in ids],
            "tech_tokens": [["ECONNRESET"] if i % 4 == 0 else [f"TOK-{i % 5}"] for i in ids],
            "entities": [entities_of(i) for i in ids]}
    if id_field == "chunk_id":
        cols.update(speaker=[SPEAKERS[i % 4] for i in ids], start_ts_ms=[i for i in ids], end_ts_ms=[i + 1 for i in ids])
    else:
        cols.update(artifact_id=[i // 2 for i in ids], kind=[KINDS[i % 3] for i in ids])
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
    at = T0 + timedelta(hours=55)
    acme, ada = {"label": "ORG", "value": "acme"}, {"label": "person", "value": "ada lovelace"}
    return [(F(entity_filters=[acme]), None), (F(speakers=["ALICE", "carol ng"]), None), (F(kinds=["action  items"]), None),
            (F(entity_filters=[acme, ada]), None), (F(entity_filters=[{"label": "org", "value": "nobody"}]), None),
            (F(entity_filters=[{"label": "product", "value": "Acme"}], speakers=["bob"]), None),
            (F(entity_filters=[acme], date_from=at - timedelta(hours=40)), None), (F(entity_filters=[ada]), CALLS[:5]),
            (F(speakers=["alice"], call_tags=["outage", "billing"]), None), (F(kinds=["summary", "notes"], date_to=at), CALLS[2:]),
            (F(entity_filters=[acme, ada], speakers=["alice", "bob"], kinds=["summary"], call_tags=["outage"],
               date_from=at - timedelta(hours=60), date_to=at + timedelta(hours=90)), CALLS[:7]),
            (F(entity_filters=[acme], speakers=["alice", "bob", "carol ng"], date_from=at - timedelta(hours=60),
               call_tags=["outage", "renewal"]), CALLS[1:8]),
            (F(entity_filters=[acme]), []), (None, CALLS[:2]), (F(), None), (F(call_tags=["outage"]), CALLS[:4])]


def assert_masks_follow(table):
    some = 0
    for filters, call_ids in filter_cases():
        got, want = table.filter_mask_device(filters, call_ids), table.filter_mask(filters, call_ids)
        if want is None:
            assert got is None, (filters, call_ids)
        else:
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (fl.mask_bytes(len(table)),)
            assert np.array_equal(got.cpu().numpy(), DenseIndex.pack_mask(want)), (table.name, filters, call_ids)
            some += int(want.any())
    return some


def test_table_masks_equal_the_host_masks_and_follow_edits(world):
    chunks, arts, cvec = world["chunks"], world["arts"], world["cvec"]
    assert assert_masks_follow(chunks) >= 6 and assert_masks_follow(arts) >= 3
    F = rt.RetrieveFilters
    # the NULL namespaces: speakers on the artifact table, kinds on the chunk table
    assert not arts.filter_mask(F(speakers=["alice"]), None).any() and not chunks.filter_mask(F(kinds=["summary"]), None).any()
    assert int(arts.filter_mask_device(F(speakers=["alice"]), None).sum()) == 0
    cols = chunks.attribute_columns()
    assert cols is chunks.attribute_columns() and cols.generation == chunks.generation     # one build per generation
    f = F(entity_filters=[{"label": "org", "value": "acme"}])
    assert chunks.filter_mask_device(f, None) is chunks.filter_mask_device(f, None)        # one mask per request
    assert chunks.filter_mask_device(f, None) is not chunks.filter_mask_device(F(entity_filters=[("org", "globex")]), None)
    assert chunks.delete([1003, 1120, 1121]) == 3
    assert_masks_follow(chunks)
    assert chunks.attribute_columns() is not cols and chunks.attribute_columns().n == len(chunks)
    late, started = table_rows("chunk_id", [1400, 37, 41, 1500], "text")                   # ids below the stored ones
    chunks.insert(cvec[300:304], late, call_started_at=started)
    assert len(chunks.entities) == len(chunks)
    assert_masks_follow(chunks)
    batch = filter_cases()
    masks, stride = chunks.filter_masks_device(batch)
    assert stride == fl.mask_bytes(len(chunks)) and tuple(masks.shape) == (len(batch), stride)
    for q, (filters, call_ids) in enumerate(batch):
        want = chunks.filter_mask(filters, call_ids)
        want = np.ones(len(chunks), dtype=bool) if want is None else want
        assert np.array_equal(masks[q].cpu().numpy(), DenseIndex.pack_mask(want)), q
    # a batch whose queries carry attribute clauses only: the attribute kernel alone, no input mask
    only = [c for c in batch[:6]] + [(None, None)]
    masks, stride = chunks.filter_masks_device(only)
    for q, (filters, call_ids) in enumerate(only):
        want = chunks.filter_mask(filters, call_ids)
        want = np.ones(len(chunks), dtype=bool) if want is None else want
        assert np.array_equal(masks[q].cpu().numpy(), DenseIndex.pack_mask(want)), q


def test_the_single_form_is_row_0_of_the_batch_form(world):
    """filter_mask_device(f, c) holds the bytes of filter_masks_device([(f, c)])[0], a second call returns the same
    tensor (the memo), and the mask is None exactly when filter_mask returns None -- for a request with call and date
    predicates only, with attribute clauses only, with both, and for the two that restrict nothing."""
    F = rt.RetrieveFilters
    at = T0 + timedelta(hours=55)
    acme = {"label": "org", "value": "acme"}
    requests = [(F(call_tags=["outage", "billing"], date_from=at - timedelta(hours=40)), CALLS[:6]),
                (F(entity_filters=[acme], speakers=["alice", "bob"]), None),
                (F(entity_filters=[acme], date_to=at + timedelta(hours=30)), CALLS[2:]),
                (F(), None), (None, CALLS[:2])]
    for table in (world["chunks"], world["arts"]):
        for filters, call_ids in requests:
            host = table.filter_mask(filters, call_ids)
            single = table.filter_mask_device(filters, call_ids)
            assert (single is None) == (host is None), (table.name, filters, call_ids)
            if single is None:
                continue
            assert table.filter_mask_device(filters, call_ids) is single, (table.name, filters, call_ids)
            batch, stride = table.filter_masks_device([(filters, call_ids)])
            assert tuple(batch.shape) == (1, stride) and batch[0].data_ptr() != single.data_ptr()
            assert np.array_equal(single.cpu().numpy(), batch[0].cpu().numpy()), (table.name, filters, call_ids)
            assert np.array_equal(single.cpu().numpy(), DenseIndex.pack_mask(host)), (table.name, filters, call_ids)
    assert world["chunks"].filter_mask(*requests[0]).any() and world["chunks"].filter_mask(*requests[2]).any()


def host_route(table, filters, call_ids):
    """What every caller did before the device route existed: the host mask, packed and uploaded."""
    mask = rt.DenseTable.filter_mask(table, filters, call_ids)
    return None if mask is None else torch.from_numpy(DenseIndex.pack_mask(mask)).to(DEV)


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
    acme = {"label": "org", "value": "Acme"}
    return [F(entity_filters=[acme]), F(speakers=["alice", "bob"]), F(kinds=["summary"]),
            F(entity_filters=[acme], call_ids=CALLS[:4]),                       # call-scoped: the listed-rows route is not taken
            F(entity_filters=[acme, {"label": "person", "value": "Ada Lovelace"}], date_from=at - timedelta(hours=50)),
            F(entity_filters=[{"label": "org", "value": "globex"}], external_id="ext-1", external_source="zoom", call_tags=["outage"]),
            F(entity_filters=[{"label": "org", "value": "nobody"}])]


def test_every_lane_and_the_response_match_the_host_route(world, monkeypatch):
    be, qvec = world["be"], world["qvec"]
    got = [(lane_answers(be, qvec, f), response(be, f)) for f in request_filters()]
    monkeypatch.setattr(rt.DenseTable, "filter_mask_device", host_route)
    want = [(lane_answers(be, qvec, f), response(be, f)) for f in request_filters()]
    for f, g, w in zip(request_filters(), got, want):
        assert g == w, f
    by_org = got[0]
    assert 0 < by_org[0][0] < len(world["chunks"]) and 0 < by_org[0][1] < len(world["arts"])
    assert by_org[0][2] and by_org[0][4] and by_org[0][6] and by_org[1]["quotes"]
    chunk_ids = world["chunks"].columns["chunk_id"]
    assert all(r["chunk_id"] % 3 == 0 and r["chunk_id"] % 4 for r in by_org[0][2]) and set(r["chunk_id"] for r in by_org[0][2]) <= set(chunk_ids)
    assert got[1][0][0] > 0 and got[1][0][1] == 0        # speakers: chunk rows, and no artifact rows (NULL namespace)
    assert got[2][0][0] == 0 and got[2][0][1] > 0        # kinds: the reverse
    assert got[3][0][2] and all(CALLS[(r["chunk_id"] * 7) % 9] in CALLS[:4] for r in got[3][0][2])
    assert got[6][0][0] == 0 and not got[6][0][2] and not got[6][1]["quotes"]


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
    assert got["counts"][0] > 0 and got["counts"][4] == 0 and got["counts"][12] == 0     # unknown entity; call_ids == []


def test_a_request_without_the_new_fields_builds_and_launches_nothing_new(world, monkeypatch):
    be, qvec, chunks, arts = world["be"], world["qvec"], world["chunks"], world["arts"]
    lib = _native.load()
    calls = {"built": 0, "launched": 0}
    real_init, real_fn = fl.AttributeColumns.__init__, lib.crag_attr_masks_host

    def counting_init(self, *a, **k):
        calls["built"] += 1
        real_init(self, *a, **k)

    class Counting:
        def __getattr__(self, name):
            if name == "crag_attr_masks_host":
                def wrapper(*a):
                    calls["launched"] += 1
                    return real_fn(*a)
                return wrapper
            return getattr(lib, name)

    monkeypatch.setattr(fl.AttributeColumns, "__init__", counting_init)
    monkeypatch.setattr(fl._native, "load", lambda: Counting())
    F = rt.RetrieveFilters
    at = T0 + timedelta(hours=55)
    for f in (None, F(), F(date_from=at), F(call_ids=CALLS[:4]), F(call_tags=["outage"], date_to=at + timedelta(hours=20)),
              F(entity_filters=[], speakers=[], kinds=None, call_tags=["billing"])):
        lane_answers(be, qvec, f)
        response(be, f)
    chunks.filter_masks_device([(F(date_from=at), None), (None, None), (F(call_tags=["outage"]), CALLS[:3])])
    assert calls == {"built": 0, "launched": 0} and chunks._attr_cols is None and arts._attr_cols is None
    response(be, F(speakers=["alice"]))                                       # and with one, both happen
    assert calls["built"] == 2 and calls["launched"] >= 2
