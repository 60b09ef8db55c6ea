"""The trigram field on the GPU: the postings csrc/crag_ngram.hip builds are EQUAL, element for element, to
ngram_csr_host (keys, post_ptr, post_pos, post_tf, doc_len, V, nnz) wherever the rows, the runs and the malformed bytes
fall against the kernel's tiles; NgramIndex.search equals tests/bm25_replay.py (ids, counts, score bits, padding) over
the HOST CSR; /retrieve with the lanes attached equals a CPU composition through the oracles."""
import numpy as np
import pytest
import torch

from bm25_oracle import Bm25Oracle
from bm25_replay import assert_equals_replay, replay_index
from cadence_rag_amd import _native
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import Bm25Index
from cadence_rag_amd.dense_index import DenseIndex
from cadence_rag_amd.ngram import TILE_BYTES, NgramIndex, ngram_csr_host, query_terms_host
from ngram_oracle import (FUZZY_QUERY, FUZZY_ROW, FUZZY_ROWS, GOLDEN, GramBm25Oracle, HostCsr, assert_csr_equal,
                          random_rows)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TILE = TILE_BYTES
CHARS = [b"a", "é".encode(), "€".encode(), "😀".encode()]          # 1, 2, 3 and 4 bytes


def device_csr(index):
    post_ptr, post_pos, post_tf = index.host_csr()
    return {"keys": index.keys, "post_ptr": post_ptr, "post_pos": post_pos, "post_tf": post_tf, "doc_len": index.doc_len}


def check_build(rows, what):
    """Build on the device, compare with the host rule; returns the host CSR."""
    want = ngram_csr_host(rows)
    index = NgramIndex.from_bytes(rows, np.arange(len(rows), dtype=np.int64) * 2 + 7, DEV)
    try:
        assert_csr_equal(device_csr(index), want, what)
        assert (index.n_terms, index.nnz, index.n_grams) == (want["keys"].size, want["post_pos"].size,
                                                             int(want["doc_len"].sum())), what
        assert np.array_equal(index.df, np.diff(want["post_ptr"])) and len(index) == len(rows)
    finally:
        index.close()
    return want


def letters(rng, n):
    return bytes(rng.choice(np.frombuffer(b"abcde", dtype=np.uint8), size=n).tolist())


def mixed(rng, n_chars):
    pieces = CHARS + [b" ", b"b", b"c", b"1"]
    return b"".join(pieces[i] for i in rng.integers(0, len(pieces), n_chars))


def tile_edge_rows():
    """Every row starts on a tile edge (each is 2 * TILE bytes); a run of five characters whose first has 1-4 bytes starts
    at every offset TILE - 12 ... TILE + 3: the start, the second and the third code point of some gram fall on either
    side of the edge in every combination."""
    rows = []
    for off in range(TILE - 12, TILE + 4):
        for first in range(4):
            run = b"".join(CHARS[(first + j) % 4] for j in range(5))
            for filler in (b" ", b"x"):
                rows.append((filler * off + run).ljust(2 * TILE, filler))
    return rows


def geometry_cases():
    rng = np.random.default_rng(99)
    cases = {
        "no rows": [],
        "one empty row": [b""],
        "empty rows first, last and in a row": [b"", b"", b"abc def", b"", b"", b"", b"xyzzy", b"", b""],
        "one row of 2 bytes": [b"ab"],
        "one row of 3 bytes": [b"abc"],
        "only rows without grams": [b"ab", b"", b"a b c", b"\xff\xfe"],
        "the host goldens": [g[0] for g in GOLDEN],
        "runs across the tile edge": tile_edge_rows(),
        "one row over three tiles": [mixed(rng, 6000)],
        "many rows in one tile": [mixed(rng, int(n)) for n in rng.integers(0, 12, 400)],
    }
    for d in (-1, 0, 1):
        cases[f"row end at the tile edge {d:+d}"] = [letters(rng, TILE + d), b"abcabc", letters(rng, 100)]
        cases[f"row end at the second tile edge {d:+d}, empty rows on it"] = [letters(rng, 2 * TILE + d), b"", b"",
                                                                             letters(rng, 50)]
        body = [mixed(rng, int(n)) for n in rng.integers(0, 200, 40)]
        total = sum(len(r) for r in body)
        pad = (d - total) % TILE or TILE
        cases[f"total length k * TILE {d:+d}"] = body + [letters(rng, pad)]
    # a multi-byte sequence cut by a row end on the tile edge: the lead is a separator in its row, the continuation bytes
    # are strays in the next
    for lead, rest in ((b"\xc3", b"\xa9"), (b"\xe2", b"\x82\xac"), (b"\xe2\x82", b"\xac"), (b"\xf0", b"\x9f\x98\x80"),
                       (b"\xf0\x9f", b"\x98\x80"), (b"\xf0\x9f\x98", b"\x80")):
        cases[f"sequence {lead.hex()}|{rest.hex()} cut on the tile edge"] = [
            letters(rng, TILE - len(lead) - 2) + b"ab" + lead, rest + b"cd", b"ab" + lead + rest + b"cd"]
    return cases


GEOMETRY = geometry_cases()


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_build_geometry(gpu, name):
    rows = GEOMETRY[name]
    if name == "one row over three tiles":
        assert 2 * TILE < len(rows[0]) <= 3 * TILE
    if name.startswith("total length"):
        assert (sum(len(r) for r in rows) - int(name.split()[-1])) % TILE == 0
    check_build(rows, name)


def test_tf_saturates_and_dl_does_not(gpu):
    want = check_build([b"a" * 65540, b"b", b"a" * 65537, b"a" * 65536], "saturation")
    assert want["post_tf"].tolist() == [65535, 65535, 65534] and want["doc_len"].tolist() == [65538, 0, 65535, 65534]


def test_key_order_up_to_the_largest_code_point(gpu):
    top = b"\xf4\x8f\xbf\xbf"
    rows = [b"aab", b"bab", b"aac", top + b"ab", b"a" + top + b"b", b"ab" + top, top * 3, b"0" + top * 2, top * 2 + b"0",
            "\u0080ab".encode(), "ab\u0080".encode()]
    want = check_build(rows, "key order")
    assert np.all(np.diff(want["keys"]) > 0) and want["keys"][-1] == (0x10FFFF << 42 | 0x10FFFF << 21 | 0x10FFFF)
    assert want["keys"].size == len(rows) and want["keys"].min() > 0


@pytest.fixture(scope="module")
def corpus(gpu):
    rows = random_rows(2025, 2000)
    ids = np.arange(len(rows), dtype=np.int64) * 3 + 50
    want = ngram_csr_host(rows)
    index = NgramIndex.from_bytes(rows, ids, DEV)
    yield rows, ids, want, index
    index.close()


def test_random_corpus(corpus):
    rows, ids, want, index = corpus
    assert_csr_equal(device_csr(index), want, "random corpus")
    assert sum(len(r) for r in rows) > 40 * TILE and want["post_tf"].max() > 3 and want["keys"].size > 1000


def test_extend_in_two_steps_equals_the_fresh_build(corpus):
    rows, ids, want, _ = corpus
    index = NgramIndex.from_bytes(rows[:700], ids[:700], DEV)
    try:
        index.extend_bytes(rows[700:1500], ids[700:1500])
        assert len(index) == 1500
        index.extend_bytes(rows[1500:], ids[1500:])
        assert_csr_equal(device_csr(index), want, "extended")
        assert np.array_equal(index.ids, ids)
        with pytest.raises(ValueError):
            index.extend_bytes([b"abc"], [int(ids[-1])])
    finally:
        index.close()


def test_text_index_equals_bytes_index(gpu):
    texts = ["Über ABC-123", "", None, "naïve café 😀😀😀"]
    index = NgramIndex(texts, [1, 2, 3, 4], DEV)
    try:
        assert_csr_equal(device_csr(index), ngram_csr_host([(t or "").encode() for t in texts]), "texts")
    finally:
        index.close()


def test_abi_errors(gpu):
    lib = gpu
    assert lib.crag_ngram_scratch_bytes(2**31, 1) == _native.CRAG_E2BIG
    assert lib.crag_ngram_scratch_bytes(2**31 - 1, 1) > 0 and lib.crag_ngram_scratch_bytes(-1, 1) == _native.CRAG_EINVAL
    text = torch.from_numpy(np.frombuffer(b"abcdefgh" * 4, dtype=np.uint8).copy()).to(DEV)
    keys, rows = torch.full((32,), -5, dtype=torch.int64, device=DEV), torch.full((32,), -5, dtype=torch.int32, device=DEV)
    dl = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(int(lib.crag_ngram_scratch_bytes(32, 3)) // 8, dtype=torch.int64, device=DEV)

    def extract(ptr, n_bytes=32):
        d_ptr = torch.tensor(ptr, dtype=torch.int64, device=DEV)
        rc = lib.crag_ngram_extract(text.data_ptr(), n_bytes, d_ptr.data_ptr(), len(ptr) - 1, keys.data_ptr(),
                                    rows.data_ptr(), dl.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, None)
        torch.cuda.synchronize()
        return rc
    # the size check needs no 2 GB buffer: it comes first and reads the argument alone
    assert extract([0, 20, 10, 32], n_bytes=2**31) == _native.CRAG_E2BIG and "2^31" in _native.last_error()
    for bad in ([0, 20, 10, 32], [1, 10, 20, 32], [0, 10, 20, 31], [0, 10, 20, 33]):
        assert extract(bad) == _native.CRAG_EINVAL, bad
        assert "text_ptr" in _native.last_error()
    assert bool((keys == -5).all()) and bool((rows == -5).all()) and bool((dl == -5).all())   # nothing was written
    assert extract([0, 10, 10, 32]) == 0
    assert dl.tolist() == [8, 0, 20] and rows.cpu().tolist() == [0] * 10 + [2] * 22
    assert lib.crag_ngram_extract(text.data_ptr() + 1, 16, scratch.data_ptr(), 1, keys.data_ptr(), rows.data_ptr(),
                                  dl.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, None) == _native.CRAG_EINVAL
    assert lib.crag_ngram_emit(None, None, None, 5, 6, 5, None, keys.data_ptr(), None, None, scratch.data_ptr(),
                               scratch.numel() * 8, None) == _native.CRAG_EINVAL


# ---- search ---------------------------------------------------------------------------------------------------------
def host(t):
    return [x.cpu().numpy() for x in t]


def check_search(index, rows, ids, want_csr, queries, k, eligible=None):
    mask, stride = None, 0
    if eligible is not None:
        packed = DenseIndex.pack_mask(eligible)
        mask = torch.from_numpy(packed).to(DEV)
        stride = packed.shape[-1] if packed.ndim == 2 else 0
    got_ids, got_sc, got_ct = host(index.search(queries, k, row_mask=mask, mask_stride=stride))
    assert got_ids.shape == (len(queries), k) and got_sc.shape == (len(queries), k) and got_ct.shape == (len(queries),)
    # the queries' terms from the HOST arrays, the replay over the HOST CSR
    terms = query_terms_host(want_csr["keys"], np.diff(want_csr["post_ptr"]), len(rows), queries)
    want = replay_index(HostCsr(want_csr, ids), *terms, k, eligible)
    assert_equals_replay(want, got_ids, got_sc, got_ct, f"k={k}")
    return got_ids, got_sc, got_ct


@pytest.mark.parametrize("k", [1, 10, 128])
def test_search_random_corpus_equals_the_replay(corpus, k):
    rows, ids, want, index = corpus
    rng = np.random.default_rng(k)
    queries = []
    for _ in range(61):
        r = rows[int(rng.integers(0, len(rows)))]
        a = int(rng.integers(0, max(len(r) - 20, 1)))
        queries.append(r[a:a + int(rng.integers(20, 61))])
    queries += [b"", b"zzzzzz qqqqq", "abc ABC é€😀 0123".encode()]
    _, _, ct = check_search(index, rows, ids, want, queries, k)
    assert ct.max() == k and ct[61] == 0 and ct[62] == 0
    shared = rng.random(len(rows)) < 0.3
    check_search(index, rows, ids, want, queries, k, shared)
    per_query = rng.random((len(queries), len(rows))) < 0.5
    per_query[3] = False
    _, _, ct = check_search(index, rows, ids, want, queries, k, per_query)
    assert ct[3] == 0


@pytest.mark.parametrize("k", [1, 10, 128])
def test_search_goldens_equals_the_replay(gpu, k):
    rows = [g[0] for g in GOLDEN]
    ids = np.arange(len(rows), dtype=np.int64) + 1
    index = NgramIndex.from_bytes(rows, ids, DEV)
    try:
        queries = [b"abc", b"abcdef", "aé€😀".encode(), b"ab\xf4\x8f\xbf\xbf", b"xyz", b"ABC-DEF abcd"]
        want = ngram_csr_host(rows)
        _, _, ct = check_search(index, rows, ids, want, queries, k)
        assert ct[0] == min(k, int(np.diff(want["post_ptr"])[np.searchsorted(want["keys"], 97 << 42 | 98 << 21 | 99)]))
        check_search(index, rows, ids, want, queries, k, np.arange(len(rows)) % 2 == 0)
    finally:
        index.close()


def test_fuzzy_query_word_lane_misses_gram_lane_finds(gpu):
    ids = np.arange(len(FUZZY_ROWS), dtype=np.int64) + 10
    words, grams = Bm25Index(FUZZY_ROWS, ids, DEV), NgramIndex(FUZZY_ROWS, ids, DEV)
    try:
        assert int(words.search([FUZZY_QUERY], 5)[2][0]) == 0
        got_ids, got_sc, got_ct = host(grams.search([FUZZY_QUERY, "ABC12345"], 5))
        assert got_ct[0] >= 2 and got_ids[0, 0] == ids[FUZZY_ROW] and got_sc[0, 0] > got_sc[0, 1]
        assert {13, 14} <= set(got_ids[1, :got_ct[1]].tolist())
    finally:
        words.close()
        grams.close()


# ---- wiring ---------------------------------------------------------------------------------------------------------
def test_retrieve_with_and_without_the_gram_lanes(gpu, monkeypatch):
    """retrieve_evidence over GpuRetrieveBackend with the gram lanes attached == the same request over a CPU composition
    whose lexical rows come from the oracles (bm25_ngram second in lane order); without them the response is the one of
    a backend that never heard of the lane; sync_ngram_lane grows the lane after add and rebuilds it after delete."""
    from datetime import datetime, timedelta
    from uuid import UUID

    from cadence_rag_amd import embeddings
    from helpers import unit_rows
    rng = np.random.default_rng(77)
    stems = ["kubernetes", "gateway", "timeout", "rollback", "ticket", "budget", "review", "latency", "deploy", "outage",
             "sprint", "ABC-123", "api-gateway", "ECONNRESET", "café", "Zürich", "数据库", "😀ok"]
    texts = [" ".join(stems[i] for i in rng.integers(0, len(stems), int(rng.integers(2, 14)))) for _ in range(330)]
    t0 = datetime(2026, 3, 1)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(6)]

    def make(name, id_field, body, rows, extra):
        n = len(rows)
        cols = {id_field: [1000 + 2 * i for i in range(n)], "call_id": [calls[i % 6]["call_id"] for i in range(n)], body: rows}
        cols.update(extra(n))
        table = rt.DenseTable(name, id_field, dim=1024, capacity=n + 64)
        table.add(unit_rows(rng, n), cols, call_started_at=[t0 + timedelta(days=i % 6) for i in range(n)],
                  call_tags={c["call_id"]: ["t%d" % (i % 2)] for i, c in enumerate(calls)})
        return table

    chunks = make("chunks", "chunk_id", "text", texts[:250], lambda n: {
        "speaker": ["S%d" % (i % 3) for i in range(n)], "start_ts_ms": [i * 10 for i in range(n)],
        "end_ts_ms": [i * 10 + 9 for i in range(n)]})
    arts = make("artifact_chunks", "artifact_chunk_id", "content", texts[250:], lambda n: {
        "artifact_id": [i // 3 for i in range(n)], "kind": ["summary"] * n})
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: False)     # the lexical lanes are what is under test
    oracles = {}

    def oracle_of(table, body, grams):   # follows the table (rows come and go below)
        key = (table.name, table.generation, grams)
        if key not in oracles:
            rows, ids = table.columns[body], table.columns[table.id_field]
            oracles[key] = GramBm25Oracle([t.encode() for t in rows], ids) if grams else Bm25Oracle(rows, ids)
        return oracles[key]

    class CpuBackend(rt.RetrieveBackend):
        grams = True

        def resolve_call_ids(self, filters): return rt._resolve_call_ids(calls, filters)

        def _rows(self, table, body, select, q, f, c, k, grams):
            m = table.filter_mask(f, c)
            orc = oracle_of(table, body, grams)
            ids, sc, n = orc.topk(orc.as_query(q) if grams else q, k, np.ones(len(table), bool) if m is None else m)
            pos = table._positions()
            return [{col: table.columns[col][pos[int(i)]] for col in select} | {"score": float(s)}
                    for i, s in zip(ids[:n], sc[:n])]

        def fetch_chunks_bm25(self, q, f, c, k): return self._rows(chunks, "text", rt.CHUNK_SELECT, q, f, c, k, False)
        def fetch_artifacts_bm25(self, q, f, c, k): return self._rows(arts, "content", rt.ARTIFACT_SELECT, q, f, c, k, False)

        def fetch_chunks_ngram(self, q, f, c, k):
            return self._rows(chunks, "text", rt.CHUNK_SELECT, q, f, c, k, True) if self.grams else None

        def fetch_artifacts_ngram(self, q, f, c, k):
            return self._rows(arts, "content", rt.ARTIFACT_SELECT, q, f, c, k, True) if self.grams else None

    class Approx(float):
        """A lane score in a debug listing: fp32 on the GPU side, fp64 on the other."""
        def __eq__(self, other): return abs(float(self) - float(other)) <= 1e-5 * max(abs(float(self)), 1.0)
        __hash__ = float.__hash__

    def rounded(resp):
        resp.pop("query_id")
        for lanes in resp.get("debug", {}).get("lanes", {}).values():
            for lane in ("bm25", "bm25_ngram"):
                for row in lanes.get(lane, []):
                    row["score"] = Approx(row["score"])
        return resp

    cases = [
        rt.RetrieveRequest(query="kubernets gatewy timout", debug=True),
        rt.RetrieveRequest(query="rollback of the api gateway", return_style="ids_only"),
        rt.RetrieveRequest(query="ABC123 ticket", debug=True, return_style="ids_only",
                           filters=rt.RetrieveFilters(call_ids=[calls[1]["call_id"], calls[4]["call_id"]])),
        rt.RetrieveRequest(query="budjet reveiw in zurich café", debug=True,
                           filters=rt.RetrieveFilters(date_from=t0 + timedelta(days=2), call_tags=["t1"]),
                           budget=rt.Budget(max_evidence_items=5, max_total_chars=300)),
        rt.RetrieveRequest(query="qq ww", debug=True),
    ]
    lanes = []
    try:
        word_lanes = dict(bm25_chunks=chunks.build_bm25_lane("text"), bm25_artifacts=arts.build_bm25_lane("content"))
        gram_lanes = dict(ngram_chunks=chunks.build_ngram_lane("text"), ngram_artifacts=arts.build_ngram_lane("content"))
        lanes = list(word_lanes.values()) + list(gram_lanes.values())
        with_grams = rt.GpuRetrieveBackend(chunks, arts, calls=calls, **word_lanes, **gram_lanes)
        without = rt.GpuRetrieveBackend(chunks, arts, calls=calls, **word_lanes)
        cpu, cpu_without = CpuBackend(), CpuBackend()
        cpu_without.grams = False
        for req in cases:
            got, want = rounded(rt.retrieve_evidence(req, with_grams)), rounded(rt.retrieve_evidence(req, cpu))
            assert got == want, req
            plain = rounded(rt.retrieve_evidence(req, without))
            assert plain == rounded(rt.retrieve_evidence(req, cpu_without))
            assert "bm25_ngram" not in repr(plain)
            if req.debug:
                for side in got["debug"]["lanes"].values():
                    assert list(side)[:2] == ["bm25", "bm25_ngram"]
            if "notes" in got:
                assert got["notes"]["retrieval"]["lanes"]["bm25_ngram"] is True
                assert plain["notes"]["retrieval"]["lanes"] == {"bm25": True, "tech_tokens": True, "dense": False}
        first = rt.retrieve_evidence(cases[0], with_grams)
        assert first["debug"]["lanes"]["chunks"]["bm25"] == [] and first["debug"]["lanes"]["chunks"]["bm25_ngram"]
        assert first["quotes"] and any(stem in first["quotes"][0]["snippet"] for stem in ("kubernetes", "gateway", "timeout"))

        # rows appended behind the lane's: sync grows it, the lane object stays
        more = [f"kubernetes gateway timeout fresh {i}" for i in range(5)]
        chunks.add(unit_rows(rng, 5), {"chunk_id": [5000 + i for i in range(5)], "call_id": [calls[0]["call_id"]] * 5,
                                       "text": more, "speaker": ["S0"] * 5, "start_ts_ms": [0] * 5, "end_ts_ms": [9] * 5},
                   call_started_at=[t0] * 5)
        before = with_grams._ngram["chunks"]
        got, want = rounded(rt.retrieve_evidence(cases[0], with_grams)), rounded(rt.retrieve_evidence(cases[0], cpu))
        assert got == want and with_grams._ngram["chunks"] is before and len(before) == 255
        assert any(q["chunk_id"] >= 5000 for q in got["quotes"])
        # rows that left: sync rebuilds it
        chunks.delete([5000, 5003, 1000])
        got, want = rounded(rt.retrieve_evidence(cases[0], with_grams)), rounded(rt.retrieve_evidence(cases[0], cpu))
        after = with_grams._ngram["chunks"]
        lanes.append(after)
        assert got == want and after is not before and len(after) == 252
        assert chunks.sync_ngram_lane(after) is after
        assert_csr_equal(device_csr(after), ngram_csr_host([t.encode() for t in chunks.columns["text"]]), "after delete")
    finally:
        for lane in lanes + list(getattr(locals().get("with_grams"), "_bm25", {}).values()):
            if hasattr(lane, "close"):
                lane.close()
