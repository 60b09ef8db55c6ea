"""Query-aware snippets without a device: token spans, the cut, the window rule in numpy against the
brute-force oracle, the 64-heaviest-terms rule, the C ABI's argument errors, and retrieve_evidence over a stub backend."""
import ctypes

import numpy as np
import pytest

import snippet_oracle as so
from bm25_clause_oracle import arrays_from_rows
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import SNIPPET_MAX_TERMS, SNIPPET_STAGE, Bm25Index, heaviest_slots, tokenize
from cadence_rag_amd.config import Settings
from cadence_rag_amd.snippets import LEAD_TOKENS, clip, cut_snippet, token_spans, windows_host


# ---- token_spans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [
    "", "   ", "Plain words, about the Connection-reset!", "roll_back  v1.2.3 (ABC-123)\n\tnext",
    "Ünïcödé İstanbul ǅ straße 東京タワー café ١٢٣ x²", "a" * 255 + " " + "b" * 256 + " c", "é" * 127 + " " + "é" * 128 + " z",
    "İ" * 200 + " tail"])
def test_token_spans_are_the_tokens_of_tokenize(text):
    spans = token_spans(text)
    assert [text[b:e].lower() for b, e in spans] == tokenize(text)
    assert all(0 <= b < e <= len(text) for b, e in spans) and spans == sorted(spans)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_a_token_over_255_bytes_has_no_span():
    text = "a" * 255 + " " + "b" * 256 + " c"
    assert token_spans(text) == [(0, 255), (513, 514)] and tokenize(text) == ["a" * 255, "c"]
    assert token_spans("é" * 128 + " z") == [(129, 130)]        # 256 bytes in 128 characters


# ---- cut_snippet ------------------------------------------------------------------------------------------------------
WORDS = " ".join(f"w{i:03d}" for i in range(400))                 # 400 tokens of 4 characters, 1 999 characters


def test_cut_snippet_cases():
    short = "it fits, whatever the window"
    assert cut_snippet(short, 3, 4, 800) == short and cut_snippet(short, -1, 0, len(short)) == short
    assert cut_snippet(WORDS, -1, 0, 800) == clip(WORDS, 800)                      # no query word: the head clip
    assert cut_snippet(WORDS, 0, 5, 800) == clip(WORDS, 800)                       # start 0 ...
    assert cut_snippet(WORDS, LEAD_TOKENS, 20, 800) == clip(WORDS, 800)            # ... and up to token 8: from character 0
    got = cut_snippet(WORDS, 300, 310, 100)
    assert got.startswith("…w292 ") and got.endswith("…") and len(got) <= 100 and "w300" in got
    assert got == clip("…" + WORDS[292 * 5:], 100)
    near_end = cut_snippet(WORDS, 399, 399, 800)                                   # the tail fits: no closing ellipsis
    assert near_end == "…" + WORDS[391 * 5:] and near_end.endswith("w399")
    assert cut_snippet(WORDS, 300, 310, 1) == "…" and cut_snippet(WORDS, 300, 310, 0) == ""
    assert cut_snippet(WORDS, 300, 310, -5) == "" and cut_snippet(WORDS, -1, 0, 1) == "…"
    assert cut_snippet(WORDS, 300, 310, 3) == "…w…"                                # a budget smaller than one token
    assert cut_snippet(WORDS, 300, 399, 40).startswith("…w292") and "w399" not in cut_snippet(WORDS, 300, 399, 40)
    assert cut_snippet(WORDS, 400, 400, 800) == clip(WORDS, 800)                   # no such token: the head clip
    padded = "  ((  " + WORDS
    assert cut_snippet(padded, 2, 2, 50) == clip(padded, 50)                       # token 0: the cut begins at character 0
    assert all(len(cut_snippet(WORDS, s, s, m)) <= m for s in (0, 9, 200, 399) for m in (1, 2, 7, 50, 799))


# ---- windows_host against the oracle ---------------------------------------------------------------------------------
@pytest.fixture()
def host_index(monkeypatch):
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)

    def build(rows, n_terms):
        row_ptr, terms, tfs, pair_off, pair_where = arrays_from_rows(rows)
        return Bm25Index.from_arrays(row_ptr, terms, tfs, n_terms, np.arange(len(rows)), "cpu", pair_off=pair_off,
                                     pair_where=pair_where)
    return build


def same_bits(got, want):
    for g, w, name in zip(got, want, ("start", "last", "score", "covered")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              w.view(np.uint32) if w.dtype == np.float32 else w), name


@pytest.mark.parametrize("window", [7, 120])
def test_windows_host_equals_the_oracle_on_the_random_case(host_index, window):
    rows, queries, pairs = so.random_case()
    ix = host_index(rows, 50)
    args = so.batch(queries, pairs)
    got = windows_host(*ix.host_csr()[:2], *ix.host_positions(), *args, window)
    same_bits(got, so.windows(rows, *args, window))
    assert (got[0] >= 0).all() and len(set(got[0].tolist())) > 20


def test_windows_host_edges(host_index):
    rows = [[9, 0, 9, 9, 1, 9, 0], [9, 9, 9], [], [1, 0, 1]]
    ix = host_index(rows, 10)
    args = so.batch([([0, 1], [1.0, 2.0]), ([5], [1.0]), ([1, 0], [1.0, 1.0])], [[0, 1, 2, 3, 0], [0], [3, 3]])
    for window in (1, 3, 4, 65535):
        got = windows_host(*ix.host_csr()[:2], *ix.host_positions(), *args, window)
        same_bits(got, so.windows(rows, *args, window))
    start, last, score, covered = windows_host(*ix.host_csr()[:2], *ix.host_positions(), *args, 3)
    assert start.tolist() == [4, -1, -1, 0, 4, -1, 0, 0] and last.tolist() == [6, 0, 0, 2, 6, 0, 2, 2]
    assert score.tolist() == [3.0, 0.0, 0.0, 3.0, 3.0, 0.0, 2.0, 2.0] and covered.tolist() == [3, 0, 0, 3, 3, 0, 3, 3]
    with pytest.raises(ValueError):
        windows_host(*ix.host_csr()[:2], *ix.host_positions(), *args, 0)


def test_the_oracle_tries_every_start():
    # one term at 5, W = 3: starts 3, 4 and 5 hold it; the answer is the occurrence, the claim's check ran over all six
    assert so.window_of([9, 9, 9, 9, 9, 0], [0], [1.5], 3) == (5, 5, np.float32(1.5), 1)
    # equal scores at two starts: the lower wins; exactly W apart is not covered together, W - 1 apart is
    assert so.window_of([0, 9, 9, 1, 9, 9, 0, 9, 9, 1], [0, 1], [1.0, 1.0], 3)[:2] == (0, 0)
    assert so.window_of([0, 9, 9, 1, 9, 9, 0, 9, 9, 1], [0, 1], [1.0, 1.0], 4)[:2] == (0, 3)
    assert so.window_of([9] * 65534 + [0, 1], [0, 1], [1.0, 1.0], 9) == (65534, 65534, np.float32(1.0), 1)
    assert so.window_of([9] * 65535 + [0], [0], [1.0], 9) == (-1, 0, np.float32(0.0), 0)


# ---- the 64 heaviest terms --------------------------------------------------------------------------------------------
def test_heaviest_slots():
    terms = np.arange(100, dtype=np.int32) * 3
    weights = np.ones(100, dtype=np.float32)
    weights[40:] = 200.0 - np.arange(60)                          # 60 slots above the cut ...
    weights[[37, 3, 25, 11, 30, 19]] = 50.0                       # ... and six equal ones for the four places left
    q_ptr = np.array([0, 100, 105, 105], dtype=np.int32)
    terms2, weights2 = np.concatenate([terms, terms[:5]]), np.concatenate([weights, weights[:5]])
    p, t, w = heaviest_slots(q_ptr, terms2, weights2, SNIPPET_MAX_TERMS)
    assert p.tolist() == [0, 64, 69, 69] and t.dtype == np.int32 and w.dtype == np.float32
    order = sorted(range(100), key=lambda i: (-float(weights[i]), int(terms[i])))[:64]
    assert t[:64].tolist() == sorted(int(terms[i]) for i in order)
    assert w[:64].tolist() == [float(weights[i]) for i in sorted(order)]
    assert t[64:].tolist() == terms[:5].tolist() and w[64:].tolist() == weights[:5].tolist()
    assert [i for i in (3, 11, 19, 25, 30, 37) if 3 * i in set(t[:64].tolist())] == [3, 11, 19, 25]   # the lower ids stay
    same = heaviest_slots(q_ptr[1:] - 100, terms[:5], weights[:5], SNIPPET_MAX_TERMS)
    assert same[0].tolist() == [0, 5, 5] and same[1] is not None and np.array_equal(same[1], terms[:5])


def test_snippet_terms_are_the_bag_reading(monkeypatch):
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    ix = Bm25Index(["alpha beta gamma delta", "beta beta epsilon"], [1, 2], "cpu", positions=True)
    ix.n, ix.df = 2, np.diff(ix.host_csr()[0])
    got = ix.snippet_terms(['+alpha -beta "gamma delta" epsilon nosuch', "beta -"])
    want = ix.query_terms(["alpha gamma delta epsilon", "beta"])
    for a, b in zip(got, want):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    over = " ".join(f"+t{i}" for i in range(17)) + " alpha"      # over the syntax's limits: tokenised as it stands
    assert np.array_equal(ix.snippet_terms([over])[1], ix.query_terms(["alpha"])[1])
    many = Bm25Index([" ".join(f"t{i}" for i in range(80))], [1], "cpu", positions=True)
    many.n, many.df = 1, np.diff(many.host_csr()[0])
    q_ptr, terms, weights = many.snippet_terms([" ".join(f"t{i}" for i in range(80)) + " t70 t71 t79"])
    assert q_ptr.tolist() == [0, 64] and terms.tolist() == list(range(61)) + [70, 71, 79]   # 3 double weights + 61 lowest ids


def test_constants_and_settings(monkeypatch):
    assert SNIPPET_MAX_TERMS == 64 and SNIPPET_STAGE >= 1024     # a 600-token chunk fits with room to spare
    assert Settings().snippet_best is False and Settings().snippet_window_tokens == 120
    monkeypatch.setenv("RETRIEVE_SNIPPET_BEST", "1")
    monkeypatch.setenv("RETRIEVE_SNIPPET_WINDOW_TOKENS", "60")
    assert Settings.from_env().snippet_best is True and Settings.from_env().snippet_window_tokens == 60
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    with pytest.raises(ValueError, match="positions"):
        Bm25Index(["a b"], [1], "cpu").snippet_windows(["a"], [[1]], 10)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _f32(*v):
    return (ctypes.c_float * len(v))(*v)


def call_snippets(lib, fake, **kw):
    """One valid call (2 queries of 2 and 1 slots, 3 pairs, n = 100, 7 terms) with overrides."""
    a = dict(post_ptr=fake, post_pos=fake, post_off=fake, post_where=fake, n=100, v=7, q_ptr=_i32(0, 2, 3),
             terms=_i32(0, 6, 3), weights=_f32(1.0, 2.0, 0.0), r_ptr=_i32(0, 2, 3), rows=_i32(0, 99, 5), nq=2, window=120,
             slot=fake, start=fake, last=fake, score=fake, covered=fake, stream=None)
    a.update(kw)
    return lib.crag_bm25_snippets_host(a["post_ptr"], a["post_pos"], a["post_off"], a["post_where"], a["n"], a["v"],
                                       a["q_ptr"], a["terms"], a["weights"], a["r_ptr"], a["rows"], a["nq"], a["window"],
                                       a["slot"], a["start"], a["last"], a["score"], a["covered"], a["stream"])


def test_cabi_argument_errors_without_a_device(native_lib):
    fake = 0x1000   # never dereferenced: every case is refused before the first HIP call
    bad_cases = [
        dict(nq=0), dict(nq=65), dict(nq=-1), dict(n=-1), dict(n=2 ** 31), dict(v=-1), dict(v=2 ** 31),
        dict(window=0), dict(window=65536), dict(window=-3),
        dict(post_off=None), dict(post_where=None), dict(post_ptr=None), dict(post_pos=None),      # NULL position arrays
        dict(q_ptr=None), dict(r_ptr=None), dict(slot=None), dict(terms=None), dict(weights=None), dict(rows=None),
        dict(start=None), dict(last=None), dict(score=None), dict(covered=None),
        dict(start=fake + 2), dict(covered=fake + 4),
        dict(q_ptr=_i32(1, 2, 3)), dict(r_ptr=_i32(1, 2, 3)), dict(q_ptr=_i32(0, 2, 1)), dict(r_ptr=_i32(0, 2, 1)),   # descend
        dict(q_ptr=_i32(0, 65, 66), terms=_i32(*[0] * 66), weights=_f32(*[1.0] * 66)),               # 65 slots
        dict(terms=_i32(0, 7, 3)), dict(terms=_i32(-1, 6, 3)),                                        # term ids
        dict(rows=_i32(0, 100, 5)), dict(rows=_i32(0, 99, -1)),                                       # rows
        dict(weights=_f32(1.0, -1.0, 0.0)), dict(weights=_f32(1.0, float("nan"), 0.0)),
        dict(weights=_f32(float("inf"), 1.0, 0.0)),
    ]
    for bad in bad_cases:
        assert call_snippets(native_lib, fake, **bad) == -1, bad            # CRAG_EINVAL
        assert b"bm25_snippets_host" in native_lib.crag_last_error(), bad
    # 64 slots pass the checks; npairs == 0: CRAG_OK, nothing enqueued (no device is touched)
    assert call_snippets(native_lib, fake, r_ptr=_i32(0, 0, 0), rows=None, start=None, last=None, score=None,
                         covered=None) == 0
    assert call_snippets(native_lib, fake, q_ptr=_i32(0, 64, 64), terms=_i32(*[6] * 64), weights=_f32(*[1.0] * 64),
                         r_ptr=_i32(0, 0, 0)) == 0


# ---- retrieve_evidence over a stub backend ----------------------------------------------------------------------------
FILLER = " ".join(f"filler{i}" for i in range(400))              # about 3 600 characters without the query word
LATE = FILLER + " the needle sits here " + " ".join(f"tail{i}" for i in range(30))
EARLY = "needle up front " + FILLER


class _StubBackend(rt.RetrieveBackend):
    """Two chunks from the word lane; snippet windows from the host rule over a host-built index."""

    def __init__(self):
        self.asked = []
        self.texts = {7: LATE, 9: EARLY, 11: "short needle text"}
        self.ix = Bm25Index(list(self.texts.values()), list(self.texts), "cpu", positions=True)
        self.ix.n, self.ix.df = len(self.texts), np.diff(self.ix.host_csr()[0])

    def fetch_chunks_bm25(self, query, filters, call_ids, limit):
        return [{"chunk_id": cid, "call_id": "c%d" % cid, "speaker": "A", "start_ts_ms": 0, "end_ts_ms": 1,
                 "text": text, "score": 1.0} for cid, text in self.texts.items()]

    def snippet_windows(self, table_name, query, ids):
        self.asked.append((table_name, query, list(ids)))
        if table_name != "chunks":
            return None
        q_ptr, terms, weights = self.ix.snippet_terms([query])
        rows = np.searchsorted(self.ix.ids, np.asarray(ids)).astype(np.int32)
        start, last, _, _ = windows_host(*self.ix.host_csr()[:2], *self.ix.host_positions(), q_ptr, terms, weights,
                                         np.array([0, len(ids)], dtype=np.int32), rows, rt.settings.snippet_window_tokens)
        return list(zip(start.tolist(), last.tolist()))


def _strip(response):
    return {k: v for k, v in response.items() if k != "query_id"}


def test_retrieve_evidence_with_the_knob_off_and_on(monkeypatch):
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    be, plain = _StubBackend(), rt.RetrieveBackend()
    plain.fetch_chunks_bm25 = be.fetch_chunks_bm25               # a backend that cannot place snippets: the default None
    req = rt.RetrieveRequest(query="needle")
    monkeypatch.setattr(rt.settings, "snippet_best", False)
    off = rt.retrieve_evidence(req, be)
    assert be.asked == [] and _strip(off) == _strip(rt.retrieve_evidence(req, plain))
    assert [q["snippet"] for q in off["quotes"]] == [clip(t, 800) for t in be.texts.values()]
    assert "needle" not in off["quotes"][0]["snippet"] and "snippet_mode" not in off["notes"]["retrieval"]

    monkeypatch.setattr(rt.settings, "snippet_best", True)
    on = rt.retrieve_evidence(req, be)
    assert be.asked == [("chunks", "needle", [7, 9, 11])]        # one question per side; the artifact side has no rows
    late, early, short = [q["snippet"] for q in on["quotes"]]
    assert "needle" in late and late.startswith("…filler393 ") and len(late) <= 800    # token 401 - 8
    assert early == clip(EARLY, 800) and short == "short needle text"
    assert on["notes"]["retrieval"]["snippet_mode"] == "best"
    on["notes"]["retrieval"].pop("snippet_mode")
    on["quotes"][0]["snippet"] = off["quotes"][0]["snippet"]
    assert _strip(on) == _strip(off)                             # nothing else moved
    # a backend that answers None keeps the head clips; the purse is charged with what was cut
    fallback = rt.retrieve_evidence(req, plain)
    assert [q["snippet"] for q in fallback["quotes"]] == [q["snippet"] for q in off["quotes"]]
    tight = rt.retrieve_evidence(rt.RetrieveRequest(query="needle", budget=rt.Budget(max_total_chars=120)), be)
    assert sum(len(q["snippet"]) for q in tight["quotes"]) <= 120 and "needle" in tight["quotes"][0]["snippet"]
