"""BM25 lane, host side: tokeniser, index builder, the oracle itself, the retrieve backend seam and the C ABI's argument
checks.  No GPU."""
import ctypes

import numpy as np
import pytest

from bm25_oracle import Bm25Oracle, tolerance
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import Bm25Index, tokenize


# ---- tokeniser ----------------------------------------------------------------------------------------------------
def test_tokenizer_cases():
    assert tokenize("We saw ECONNRESET in api-gateway.") == ["we", "saw", "econnreset", "in", "api", "gateway"]
    assert tokenize("Let's roll back version 1.2.3.") == ["let", "s", "roll", "back", "version", "1", "2", "3"]
    assert tokenize("ticket ABC-123, file_name.py; x_y") == ["ticket", "abc", "123", "file", "name", "py", "x", "y"]
    assert tokenize("HTTP500 http500 Http500") == ["http500"] * 3
    assert tokenize("") == [] and tokenize("  ...--__  ") == []
    assert tokenize("Größe naïve ДОБРЫЙ день 東京タワー") == ["größe", "naïve", "добрый", "день", "東京タワー"]
    assert tokenize("a" * 255 + " " + "b" * 256 + " " + "c" * 300 + " ok") == ["a" * 255, "ok"]
    assert tokenize("é" * 127 + " " + "é" * 128) == ["é" * 127]          # 254 and 256 UTF-8 bytes


def test_tokenizer_is_isalnum_per_character():
    """The regular expression of the implementation against the definition, over the BMP and a few planes beyond."""
    chars = [chr(c) for c in list(range(0, 0x3000)) + list(range(0xFF00, 0x10000)) + list(range(0x1D400, 0x1D800))
             if not 0xD800 <= c < 0xE000]
    text = "".join(chars)
    want, run = [], []
    for ch in text:
        if ch.isalnum():
            run.append(ch)
        elif run:
            want.append("".join(run).lower())
            run = []
    if run:
        want.append("".join(run).lower())
    assert tokenize(text) == [t for t in want if len(t.encode("utf-8")) <= 255]


# ---- builder ------------------------------------------------------------------------------------------------------
CORPUS = ["We saw ECONNRESET in api-gateway.", "Let's roll back version 1.2.3.", "Action item: file ticket ABC-123.",
          "", "the api api API gateway saw saw it", "roll roll roll back", "...", "ticket 123 in the gateway"]
IDS = [10, 11, 15, 16, 20, 21, 30, 31]


@pytest.fixture()
def host_index(monkeypatch):
    """The builder without a device: the upload is the only step that needs one."""
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    return lambda texts, ids: Bm25Index(texts, ids, "cpu")


def test_builder_invariants(host_index):
    ix = host_index(CORPUS, IDS)
    post_ptr, post_pos, post_tf = ix.host_csr()
    v = len(ix.vocab)
    assert post_ptr.dtype == np.int64 and post_pos.dtype == np.int32 and post_tf.dtype == np.uint16
    assert post_ptr.shape == (v + 1,) and post_ptr[0] == 0 and post_ptr[-1] == post_pos.size
    for t in range(v):
        pos = post_pos[post_ptr[t]:post_ptr[t + 1]]
        assert pos.size >= 1 and np.all(np.diff(pos) > 0)                # ascending, distinct
    assert int(post_tf.sum()) == int(ix.doc_len.sum())                   # sum tf = sum dl
    assert ix.doc_len.tolist() == [len(tokenize(t)) for t in CORPUS]
    # df = list lengths = rows that hold the term
    for tok, t in ix.vocab.items():
        assert post_ptr[t + 1] - post_ptr[t] == sum(tok in tokenize(text) for text in CORPUS)
    # term ids in order of first appearance
    assert [tok for tok, _ in sorted(ix.vocab.items(), key=lambda kv: kv[1])][:6] == tokenize(CORPUS[0])
    api = ix.vocab["api"]
    assert post_pos[post_ptr[api]:post_ptr[api + 1]].tolist() == [0, 4]
    assert post_tf[post_ptr[api]:post_ptr[api + 1]].tolist() == [1, 3]


def test_extend_equals_fresh_build(host_index):
    grown = host_index(CORPUS[:3], IDS[:3])
    grown._append(CORPUS[3:6], IDS[3:6])
    grown._append(CORPUS[6:], IDS[6:])
    fresh = host_index(CORPUS, IDS)
    assert grown.vocab == fresh.vocab
    for a, b in zip(grown.host_csr(), fresh.host_csr()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for name in ("row_ptr", "row_terms", "row_tf", "doc_len", "ids"):
        assert np.array_equal(getattr(grown, name), getattr(fresh, name)), name


def test_ids_must_ascend(host_index):
    with pytest.raises(ValueError):
        host_index(["a", "b"], [2, 2])
    with pytest.raises(ValueError):
        host_index(["a", "b"], [3, 1])
    ix = host_index(["a", "b"], [1, 2])
    with pytest.raises(ValueError):
        ix._append(["c"], [2])
    with pytest.raises(ValueError):
        host_index(["a"], [1, 2])


def test_query_terms_weights(host_index):
    ix = host_index(CORPUS, IDS)
    ix.n, ix.df = len(CORPUS), np.diff(ix.host_csr()[0])
    q_ptr, terms, w = ix.query_terms(["gateway api api nosuchword", "", "zzz"])
    assert q_ptr.tolist() == [0, 2, 2, 2] and terms.dtype == np.int32 and w.dtype == np.float32
    assert terms.tolist() == sorted([ix.vocab["api"], ix.vocab["gateway"]])
    n = 8.0
    idf = lambda df: np.log(1.0 + (n - df + 0.5) / (df + 0.5))
    want = {ix.vocab["api"]: 2 * idf(2) * 2.2, ix.vocab["gateway"]: idf(3) * 2.2}
    assert [float(x) for x in w] == [float(np.float32(want[t])) for t in terms.tolist()]


# ---- the oracle against numbers written out by hand -----------------------------------------------------------------
def test_oracle_three_row_example():
    """rows "a b" (dl 2), "a a c" (dl 3), "d" (dl 1): N = 3, avgdl = 2.
    idf(a) = ln(1 + 1.5 / 2.5) = ln 1.6;  idf(d) = ln(1 + 2.5 / 1.5) = ln(8 / 3).
    row 0, a: tf 1, k1 * (0.25 + 0.75 * 2 / 2) = 1.2    -> 2.2 * 1 / 2.2  = 1           -> ln 1.6
    row 1, a: tf 2, k1 * (0.25 + 0.75 * 3 / 2) = 1.65   -> 2.2 * 2 / 3.65 = 4.4 / 3.65  -> ln 1.6 * 4.4 / 3.65
    row 2, d: tf 1, k1 * (0.25 + 0.75 * 1 / 2) = 0.75   -> 2.2 * 1 / 1.75               -> ln(8/3) * 2.2 / 1.75"""
    o = Bm25Oracle(["a b", "a a c", "d"], [7, 8, 9])
    s, t = o.scores("a")
    assert t == 1
    assert s[0] == pytest.approx(0.47000362924573558, rel=1e-14)
    assert s[1] == pytest.approx(0.47000362924573558 * 4.4 / 3.65, rel=1e-14)
    assert s[1] == pytest.approx(0.56657971744691413, rel=1e-12)
    assert s[2] == 0.0
    ids, sc, n = o.topk("a", 5)
    assert ids.tolist() == [8, 7, -1, -1, -1] and n == 2 and np.isnan(sc[2:]).all()
    s, t = o.scores("d a d")                       # qtf(d) = 2
    assert t == 2
    assert s[2] == pytest.approx(2 * 0.98082925301172619 * 2.2 / 1.75, rel=1e-14)
    assert s[2] == pytest.approx(2.4660849790009121, rel=1e-12)
    assert o.topk("d a d", 2)[0].tolist() == [9, 8]
    assert o.topk("d a d", 2, eligible=[True, True, False])[0].tolist() == [8, 7]
    assert o.topk("nothing known", 3)[2] == 0
    assert tolerance(2) == 2 * 11 * 2.0 ** -24


# ---- GpuRetrieveBackend with a lane object --------------------------------------------------------------------------
class _StubTable:
    id_field = "chunk_id"
    generation = 0

    def __init__(self):
        self.columns = {"chunk_id": [100, 101, 102], "call_id": ["c1", "c1", "c2"], "speaker": ["A", "B", "A"],
                        "start_ts_ms": [0, 5, 10], "end_ts_ms": [5, 10, 15], "text": ["x", "y", "z"]}

    def __len__(self): return 3
    def filter_mask(self, filters, call_ids): return None if call_ids is None else np.array([True, False, True])
    def _positions(self): return {100: 0, 101: 1, 102: 2}
    def sync_bm25_lane(self, lane): return lane


class _StubLane:
    device = "cpu"

    def __init__(self): self.calls = []

    def search(self, query_texts, k, row_mask=None, mask_stride=0, stream=0):
        self.calls.append((list(query_texts), k, None if row_mask is None else row_mask.numpy().tolist(), mask_stride))
        ids = np.full((1, k), -1, dtype=np.int64)
        sc = np.full((1, k), np.nan, dtype=np.float32)
        ids[0, :2], sc[0, :2] = [102, 100], [1.5, 0.25]
        return ids, sc, np.array([2], dtype=np.int32)


def test_backend_with_a_lane_object_and_with_a_callable():
    table, lane = _StubTable(), _StubLane()
    be = rt.GpuRetrieveBackend(table, _StubTable(), bm25_chunks=lane,
                               bm25_artifacts=lambda q, f, c, k: [{"artifact_chunk_id": 5, "score": 2.0}][:k])
    rows = be.fetch_chunks_bm25("what about z", None, None, 50)
    assert [set(r) for r in rows] == [set(rt.CHUNK_SELECT) | {"score"}] * 2
    assert [(r["chunk_id"], r["text"], r["score"]) for r in rows] == [(102, "z", 1.5), (100, "x", 0.25)]
    assert lane.calls == [(["what about z"], 50, None, 0)]
    be.fetch_chunks_bm25("q", None, ["c1"], 500)       # k is capped at CRAG_MAX_K, the filter arrives as a packed mask
    assert lane.calls[-1] == (["q"], 128, [0b101, 0, 0, 0], 0)
    assert be.fetch_artifacts_bm25("q", None, None, 10) == [{"artifact_chunk_id": 5, "score": 2.0}]
    assert rt.GpuRetrieveBackend(table, table).fetch_chunks_bm25("q", None, None, 10) == []


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_cabi_argument_errors_without_a_device(native_lib):
    lib = native_lib
    assert hasattr(lib, "crag_bm25_lane_host") and hasattr(lib, "crag_bm25_scratch_bytes")
    assert lib.crag_bm25_scratch_bytes(16384, 64, 50) >= 64 * 50 * 8 + 64 * 4
    assert lib.crag_bm25_scratch_bytes(16385, 64, 128) > lib.crag_bm25_scratch_bytes(16384, 64, 128)   # a second range
    assert lib.crag_bm25_scratch_bytes(-1, 1, 1) == -1 and lib.crag_bm25_scratch_bytes(10, 65, 1) == -1
    assert lib.crag_bm25_scratch_bytes(10, 1, 129) == -1 and lib.crag_bm25_scratch_bytes(2 ** 31, 1, 1) == -1
    q_ptr = (ctypes.c_int32 * 2)(0, 1)
    terms = (ctypes.c_int32 * 1)(0)
    w = (ctypes.c_float * 1)(1.0)
    fake = 0x1000   # never dereferenced: every case below is refused before the first HIP call

    def call(**kw):
        a = dict(post_ptr=fake, post_pos=fake, post_tf=fake, doc_len=fake, ids=None, n=10, v=4, avgdl=2.0,
                 q_ptr=q_ptr, terms=terms, w=w, nq=1, k=10, mask=None, stride=0, slot=fake, scratch=fake,
                 scratch_bytes=1 << 20, out_ids=fake, out_sc=fake, out_ct=fake)
        a.update(kw)
        return lib.crag_bm25_lane_host(a["post_ptr"], a["post_pos"], a["post_tf"], a["doc_len"], a["ids"], a["n"], a["v"],
                                       ctypes.c_float(a["avgdl"]), a["q_ptr"], a["terms"], a["w"], a["nq"], a["k"],
                                       a["mask"], a["stride"], a["slot"], a["scratch"], a["scratch_bytes"], a["out_ids"],
                                       a["out_sc"], a["out_ct"], None)
    for bad in (dict(post_ptr=None), dict(post_pos=None), dict(post_tf=None), dict(doc_len=None), dict(q_ptr=None),
                dict(slot=None), dict(scratch=None), dict(out_ids=None), dict(out_sc=None), dict(out_ct=None),
                dict(terms=None), dict(w=None),
                dict(nq=65), dict(nq=-1), dict(k=0), dict(k=129), dict(n=-1), dict(n=2 ** 31), dict(v=-1),
                dict(avgdl=0.0), dict(avgdl=float("nan")), dict(scratch_bytes=8), dict(scratch=fake + 4),
                dict(mask=fake, stride=2), dict(mask=fake + 1), dict(mask=fake, stride=4 * 100, n=4000),
                dict(q_ptr=(ctypes.c_int32 * 2)(1, 1)), dict(q_ptr=(ctypes.c_int32 * 2)(0, -1)),
                dict(terms=(ctypes.c_int32 * 1)(4)), dict(terms=(ctypes.c_int32 * 1)(-1)),
                dict(q_ptr=(ctypes.c_int32 * 2)(0, 2), terms=(ctypes.c_int32 * 2)(1, 1), w=(ctypes.c_float * 2)(1, 1)),
                dict(w=(ctypes.c_float * 1)(0.0)), dict(w=(ctypes.c_float * 1)(float("inf")))):
        assert call(**bad) == -1, bad                                   # CRAG_EINVAL
        assert b"bm25_lane_host" in lib.crag_last_error(), bad
    assert call(nq=0) == 0                                              # nothing to do, nothing enqueued
