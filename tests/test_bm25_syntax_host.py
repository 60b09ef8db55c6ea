"""BM25 clause syntax, host side: the parser, the positional postings, the clause arrays, the setting and
the retrieve backend's seam.  No GPU."""
import ctypes

import numpy as np
import pytest

from bm25_clause_oracle import ClauseOracle, arrays_from_rows, clauses_of, holds_phrase, packed
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import (EXC_PHRASE, EXC_TERM, MATCH_NOTHING, REQ_PHRASE, REQ_TERM, Bm25Index, ParsedQuery,
                                  QuerySyntaxError, parse_query, tokenize)
from cadence_rag_amd.config import Settings

R, X, P, XP = REQ_TERM, EXC_TERM, REQ_PHRASE, EXC_PHRASE

# query -> (clauses, bag, text)
PARSER_TABLE = [
    ("timeout staging", [], ["timeout", "staging"], "timeout staging"),
    ('+timeout -staging "connection reset"', [(R, ("timeout",)), (X, ("staging",)), (P, ("connection", "reset"))],
     ["timeout", "connection", "reset"], "timeout connection reset"),
    ("a-b", [], ["a", "b"], "a-b"),                                  # a prefix only at the start of an item
    ("a+b x -", [], ["a", "b", "x"], "a+b x"),
    ("+a-b", [(R, ("a",)), (R, ("b",))], ["a", "b"], "a-b"),
    ("-a-b c", [(X, ("a",)), (X, ("b",))], ["c"], "c"),
    ('-"x y"', [(XP, ("x", "y"))], [], ""),
    ('+"x y"', [(P, ("x", "y"))], ["x", "y"], "x y"),
    ('"x"', [(R, ("x",))], ["x"], "x"),
    ('-"x"', [(X, ("x",))], [], ""),
    ('""', [], [], ""),
    ('"..."', [], [], ""),
    ('foo "bar baz', [(P, ("bar", "baz"))], ["foo", "bar", "baz"], "foo bar baz"),       # an unclosed quote
    ("+", [], [], ""),
    ("+ foo", [], ["foo"], "foo"),                                    # the prefix must touch its item
    ("foo +", [], ["foo"], "foo"),
    ('"+a -b"', [(P, ("a", "b"))], ["a", "b"], "+a -b"),              # a prefix inside quotes is text
    ("--a", [(X, ("a",))], [], ""),                                   # one prefix; the second is text
    ("+-a", [(R, ("a",))], ["a"], "-a"),
    ('a"b c"d', [(P, ("b", "c"))], ["a", "b", "c", "d"], "a b c d"),  # a quote ends an unquoted item
    ('x\t+y\n-"z w"', [(R, ("y",)), (XP, ("z", "w"))], ["x", "y"], "x y"),
    ("field:value (a OR b)* c~2", [], ["field", "value", "a", "or", "b", "c", "2"], "field:value (a OR b)* c~2"),
    ("+Größe -ДОБРЫЙ \"東京タワー Naïve\"", [(R, ("größe",)), (X, ("добрый",)), (P, ("東京タワー", "naïve"))],
     ["größe", "東京タワー", "naïve"], "Größe 東京タワー Naïve"),
    ("+" + "b" * 256 + " +ok", [(R, ("ok",))], ["ok"], "ok"),         # an overlong token is dropped by tokenize
    ('"' + "b" * 256 + ' ok"', [(R, ("ok",))], ["ok"], "b" * 256 + " ok"),
    ("", [], [], ""),
    (None, [], [], ""),
]


@pytest.mark.parametrize("case", PARSER_TABLE, ids=[repr(c[0])[:40] for c in PARSER_TABLE])
def test_parser_table(case):
    text, clauses, bag, kept = case
    got = parse_query(text)
    assert isinstance(got, ParsedQuery)
    assert list(got.clauses) == clauses and list(got.bag) == bag and got.text == kept
    assert got.has_constraints == bool(clauses)


def test_parser_limits():
    assert len(parse_query(" ".join(f"+t{i}" for i in range(16))).clauses) == 16
    with pytest.raises(QuerySyntaxError):
        parse_query(" ".join(f"+t{i}" for i in range(17)))
    with pytest.raises(QuerySyntaxError):
        parse_query("+a-b-c-d-e-f-g-h-i -j-k-l-m-n-o-p-q")           # 9 + 8 clauses from two items
    assert len(parse_query(" ".join(f'-"x{i} y"' for i in range(16)) + " opt ional").clauses) == 16   # optional: no clause
    assert parse_query('"a b c d e f g h"').clauses == ((P, tuple("abcdefgh")),)
    with pytest.raises(QuerySyntaxError):
        parse_query('"a b c d e f g h i"')
    with pytest.raises(QuerySyntaxError):
        parse_query('-"a b c d e f g h i"')
    assert issubclass(QuerySyntaxError, ValueError)


CORPUS = ["We saw ECONNRESET in api-gateway.", "Let's roll back version 1.2.3.", "Action item: file ticket ABC-123.",
          "", "the api api API gateway saw saw it", "roll roll roll back", "...", "ticket 123 in the gateway",
          "connection reset by peer then the connection was reset", "reset connection"]
IDS = [10, 11, 15, 16, 20, 21, 30, 31, 40, 41]


@pytest.fixture()
def host_index(monkeypatch):
    """The builder without a device: the upload is the only step that needs one."""
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    return lambda texts, ids, **kw: Bm25Index(texts, ids, "cpu", **kw)


def test_plain_strings_parse_to_todays_bag(host_index):
    ix = host_index(CORPUS, IDS)
    ix.n, ix.df = len(CORPUS), np.diff(ix.host_csr()[0])
    queries = ["gateway api api nosuchword", "", "zzz", "roll-back version:1.2.3 (ticket)", "Where is ABC-123?"]
    parsed = [parse_query(q) for q in queries]
    assert not any(p.has_constraints for p in parsed)
    assert [list(p.bag) for p in parsed] == [tokenize(q) for q in queries]
    for a, b in zip(ix.query_terms([" ".join(p.bag) for p in parsed]), ix.query_terms(queries)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                     b.view(np.uint32) if b.dtype == np.float32 else b)


def check_positions(ix, texts):
    """Every posting's positions equal a brute-force scan of tokenize(row)."""
    post_ptr, post_pos, post_tf = ix.host_csr()
    post_off, post_where = ix.host_positions()
    assert post_off.dtype == np.int64 and post_where.dtype == np.uint16
    assert post_off.shape == (post_pos.size + 1,) and post_off[0] == 0 and post_off[-1] == post_where.size
    assert post_where.size == sum(len(tokenize(t)) for t in texts)          # 2 bytes per token
    for tok, t in ix.vocab.items():
        for j in range(post_ptr[t], post_ptr[t + 1]):
            want = [p for p, x in enumerate(tokenize(texts[post_pos[j]])) if x == tok]
            got = post_where[post_off[j]:post_off[j + 1]].tolist()
            assert got == want and len(got) == post_tf[j], (tok, int(post_pos[j]))


def test_positional_csr_of_a_text_corpus(host_index):
    ix = host_index(CORPUS, IDS, positions=True)
    check_positions(ix, CORPUS)
    plain = host_index(CORPUS, IDS)
    for a, b in zip(ix.host_csr(), plain.host_csr()):                       # positions change nothing else
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert not plain.positions
    with pytest.raises(ValueError):
        plain.host_positions()


def test_extend_keeps_positions_equal_to_a_fresh_build(host_index):
    grown = host_index(CORPUS[:3], IDS[:3], positions=True)
    grown._append(CORPUS[3:6], IDS[3:6])
    grown._append(CORPUS[6:], IDS[6:])
    fresh = host_index(CORPUS, IDS, positions=True)
    check_positions(grown, CORPUS)
    for name in ("pair_off", "pair_where", "row_ptr", "row_terms", "row_tf"):
        assert np.array_equal(getattr(grown, name), getattr(fresh, name)), name
    for a, b in zip(grown.host_positions(), fresh.host_positions()):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_positions_at_or_above_65535_are_not_indexed(host_index):
    ix = host_index(["x " * 65534 + "a b c"], [1], positions=True)
    _, _, post_tf = ix.host_csr()
    post_off, post_where = ix.host_positions()
    where = {tok: post_where[post_off[t]:post_off[t + 1]].tolist() for tok, t in ix.vocab.items()}
    assert where["a"] == [65534] and where["b"] == [] and where["c"] == [] and len(where["x"]) == 65534
    assert post_tf[ix.vocab["b"]] == 1 and ix.doc_len[0] == 65537


def test_from_arrays_round_trips_pairs(monkeypatch):
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    rows = [[0, 1, 0], [], [2, 2, 2, 1], [1], [0, 1, 1, 0, 2]]
    row_ptr, terms, tfs, pair_off, pair_where = arrays_from_rows(rows)
    ix = Bm25Index.from_arrays(row_ptr, terms, tfs, 3, np.arange(5), "cpu", pair_off=pair_off, pair_where=pair_where)
    assert ix.positions and np.array_equal(ix.pair_off, pair_off) and np.array_equal(ix.pair_where, pair_where)
    assert ix.pair_where.dtype == np.uint16 and ix.pair_off.dtype == np.int64
    post_ptr, post_pos, post_tf = ix.host_csr()
    post_off, post_where = ix.host_positions()
    for t in range(3):
        for j in range(post_ptr[t], post_ptr[t + 1]):
            want = [p for p, x in enumerate(rows[post_pos[j]]) if x == t]
            assert post_where[post_off[j]:post_off[j + 1]].tolist() == want and post_tf[j] == len(want)
    assert not Bm25Index.from_arrays(row_ptr, terms, tfs, 3, np.arange(5), "cpu").positions
    with pytest.raises(ValueError):
        Bm25Index.from_arrays(row_ptr, terms, tfs, 3, np.arange(5), "cpu", pair_off=pair_off)
    with pytest.raises(ValueError):
        Bm25Index.from_arrays(row_ptr, terms, tfs, 3, np.arange(5), "cpu", pair_off=pair_off[:-1], pair_where=pair_where)


def test_clause_arrays(host_index):
    ix = host_index(CORPUS, IDS, positions=True)
    v = ix.vocab
    parsed = [parse_query('+api -gateway "connection reset"'), parse_query("plain words"),
              parse_query('+nosuchword api'), parse_query('-nosuchword -"no such" "such api" -saw'),
              parse_query('"reset nosuchword"')]
    c_ptr, c_kind, ct_ptr, ct_terms = ix.clause_arrays(parsed)
    assert all(a.dtype == np.int32 for a in (c_ptr, c_kind, ct_ptr, ct_terms))
    assert c_ptr.tolist() == [0, 3, 3, 4, 6, 7]
    assert c_kind.tolist() == [R, X, P, MATCH_NOTHING, MATCH_NOTHING, X, MATCH_NOTHING]
    assert ct_ptr.tolist() == [0, 1, 2, 4, 4, 4, 5, 5]
    assert ct_terms.tolist() == [v["api"], v["gateway"], v["connection"], v["reset"], v["saw"]]
    with pytest.raises(ValueError, match="positions"):
        host_index(CORPUS, IDS).clause_arrays([parse_query('"connection reset"')])
    assert host_index(CORPUS, IDS).clause_arrays([parse_query("+api -saw")])[1].tolist() == [R, X]


def test_the_oracle_on_rows_written_out_by_hand(host_index):
    ix = host_index(CORPUS, IDS, positions=True)
    rows = [[ix.vocab[t] for t in tokenize(text)] for text in CORPUS]
    orc = ClauseOracle(rows)

    def passing(query, in_mask=None):
        return np.flatnonzero(orc.passes(clauses_of(parse_query(query), ix.vocab.get), in_mask)).tolist()
    assert passing('"connection reset"') == [8] and passing('-"connection reset" reset') == [0, 1, 2, 3, 4, 5, 6, 7, 9]
    assert passing('+connection +reset') == [8, 9] and passing('+connection -peer') == [9]
    assert passing('"roll back"') == [1, 5] and passing('"roll roll back"') == [5] and passing('"back roll"') == []
    assert passing('"api api api"') == [4] and passing('"saw saw it"') == [4] and passing('"it we"') == []
    assert passing('+nosuchword') == [] and passing('-nosuchword') == list(range(10)) and passing('"api nosuchword"') == []
    assert passing('+gateway', np.arange(10) != 4) == [0, 7]
    assert holds_phrase([1, 2, 1], (1, 2, 1)) and not holds_phrase([1, 2, 2, 1], (1, 2, 1))
    assert holds_phrase([1, 1, 2, 1], (1, 2, 1)) and not holds_phrase([1], (1, 1)) and holds_phrase([1] * 600, (1, 1))
    assert holds_phrase([0] * 65533 + [1, 2], (1, 2)) and not holds_phrase([0] * 65534 + [1, 2], (1, 2))
    bits = packed(np.array([[True] * 9 + [False], [False] * 9 + [True]]), 8)
    assert bits.tolist() == [0xFF, 0x01, 0, 0, 0, 0, 0, 0, 0x00, 0x02, 0, 0, 0, 0, 0, 0]


def test_setting_defaults_off(monkeypatch):
    assert Settings().bm25_query_syntax is False
    monkeypatch.setenv("BM25_QUERY_SYNTAX", "1")
    assert Settings.from_env().bm25_query_syntax is True


# ---- GpuRetrieveBackend: which lane is asked what -------------------------------------------------------------------
class _StubTable:
    id_field = "chunk_id"
    generation = 0

    def __init__(self):
        self.columns = {"chunk_id": [100, 101, 102], "call_id": ["c1", "c1", "c2"], "speaker": ["A", "B", "A"],
                        "start_ts_ms": [0, 5, 10], "end_ts_ms": [5, 10, 15], "text": ["x", "y", "z"]}

    def __len__(self): return 3
    def filter_mask(self, filters, call_ids): return None
    def _positions(self): return {100: 0, 101: 1, 102: 2}
    def sync_bm25_lane(self, lane): return lane
    def sync_ngram_lane(self, lane): return lane


class _StubLane:
    device = "cpu"

    def __init__(self): self.calls = []

    def _rows(self, how, query_texts, k):
        self.calls.append((how, list(query_texts)))
        ids = np.full((1, k), -1, dtype=np.int64)
        sc = np.full((1, k), np.nan, dtype=np.float32)
        ids[0, :1], sc[0, :1] = [101], [1.0]
        return ids, sc, np.array([1], dtype=np.int32)

    def search(self, query_texts, k, row_mask=None, mask_stride=0, stream=0): return self._rows("search", query_texts, k)
    def search_query(self, query_texts, k, row_mask=None, mask_stride=0, stream=0): return self._rows("search_query", query_texts, k)


def test_backend_routes_the_lanes_by_the_setting(monkeypatch, caplog):
    word, gram, seen = _StubLane(), _StubLane(), []
    be = rt.GpuRetrieveBackend(_StubTable(), _StubTable(), bm25_chunks=word, ngram_chunks=gram,
                               bm25_artifacts=lambda q, f, c, k: seen.append(("word", q)) or [],
                               ngram_artifacts=lambda q, f, c, k: seen.append(("gram", q)) or [])
    query = '+timeout -staging "connection  reset" plain'
    over = " ".join(f"+t{i}" for i in range(17))

    def ask(q):
        word.calls.clear(); gram.calls.clear(); seen.clear()
        assert [r["chunk_id"] for r in be.fetch_chunks_bm25(q, None, None, 10)] == [101]
        assert [r["chunk_id"] for r in be.fetch_chunks_ngram(q, None, None, 10)] == [101]
        be.fetch_artifacts_bm25(q, None, None, 10)
        be.fetch_artifacts_ngram(q, None, None, 10)
        return word.calls, gram.calls, seen
    monkeypatch.setattr(rt.settings, "bm25_query_syntax", False)
    assert ask(query) == ([("search", [query])], [("search", [query])], [("word", query), ("gram", query)])
    monkeypatch.setattr(rt.settings, "bm25_query_syntax", True)
    stripped = "timeout connection  reset plain"
    # the word lane parses the raw string itself; a callable word lane (pg_search's rows) is handed the raw string too
    assert ask(query) == ([("search_query", [query])], [("search", [stripped])], [("word", query), ("gram", stripped)])
    # over the clause limit: the bag reading of the raw string on every lane, logged once for the request
    with caplog.at_level("WARNING", logger=rt.__name__):
        assert ask(over) == ([("search", [over])], [("search", [over])], [("word", over), ("gram", over)])
    assert len([r for r in caplog.records if "query syntax" in r.getMessage()]) == 1


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def einval_cases(fake):
    """Every refusal the header lists, as overrides of one valid call (term + phrase, n = 100, 7 terms)."""
    return [dict(c_ptr=None), dict(slot=None), dict(out=None), dict(post_ptr=None), dict(post_pos=None),
            dict(c_kind=None), dict(ct_ptr=None), dict(ct_terms=None),
            dict(nq=0), dict(nq=65), dict(nq=-1), dict(n=-1), dict(n=2 ** 31), dict(v=-1), dict(v=2 ** 31),
            dict(stride=8), dict(stride=18), dict(stride=-4), dict(stride=2 ** 32 + 4), dict(out=fake + 2),
            dict(in_mask=fake, in_stride=8), dict(in_mask=fake, in_stride=18), dict(in_mask=fake + 1),
            dict(c_ptr=_i32(1, 2)), dict(c_ptr=_i32(0, -1)), dict(ct_ptr=_i32(1, 2, 4)), dict(ct_ptr=_i32(0, 3, 2)),
            dict(c_kind=_i32(0, 5)), dict(c_kind=_i32(-1, 2)),
            dict(ct_terms=_i32(7, 1, 2)), dict(ct_terms=_i32(0, 1, -1)),
            dict(ct_ptr=_i32(0, 0, 2), ct_terms=_i32(1, 2)),                                # a term clause without a term
            dict(c_kind=_i32(1, 2), ct_ptr=_i32(0, 2, 4), ct_terms=_i32(0, 1, 2, 3)),       # ... and with two
            dict(c_kind=_i32(0, 4)),                                                        # kind 4 with terms
            dict(ct_ptr=_i32(0, 1, 2), ct_terms=_i32(0, 1)),                                # a phrase of one term
            dict(c_kind=_i32(0, 3), ct_ptr=_i32(0, 1, 10), ct_terms=_i32(*range(7), 0, 1, 2)),   # ... and of nine
            dict(c_ptr=_i32(0, 17), c_kind=_i32(*[0] * 17), ct_ptr=_i32(*range(18)), ct_terms=_i32(*[0] * 17)),
            dict(post_off=None), dict(post_where=None)]                                     # a phrase without positions


def call_clause_masks(lib, fake, **kw):
    a = dict(post_ptr=fake, post_pos=fake, post_off=fake, post_where=fake, n=100, v=7, c_ptr=_i32(0, 2),
             c_kind=_i32(0, 2), ct_ptr=_i32(0, 1, 3), ct_terms=_i32(0, 1, 2), nq=1, in_mask=None, in_stride=0, slot=fake,
             out=fake, stride=16, stream=None)
    a.update(kw)
    return lib.crag_bm25_clause_masks_host(a["post_ptr"], a["post_pos"], a["post_off"], a["post_where"], a["n"], a["v"],
                                           a["c_ptr"], a["c_kind"], a["ct_ptr"], a["ct_terms"], a["nq"], a["in_mask"],
                                           a["in_stride"], a["slot"], a["out"], a["stride"], a["stream"])


def test_cabi_argument_errors_without_a_device(native_lib):
    fake = 0x1000   # never dereferenced: every case is refused before the first HIP call
    for bad in einval_cases(fake):
        assert call_clause_masks(native_lib, fake, **bad) == -1, bad        # CRAG_EINVAL
        assert b"bm25_clause_masks_host" in native_lib.crag_last_error(), bad
    # n_rows == 0 with no bytes to write: CRAG_OK, nothing enqueued
    assert call_clause_masks(native_lib, fake, n=0, stride=0, post_ptr=None, post_pos=None, out=None) == 0
