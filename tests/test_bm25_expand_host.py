"""Prefix and fuzzy items of the BM25 lane, host side: the parser with `expand`, the matching rule on
hand-written cases, the weight rule, the argument checks of the two C entries, the setting and the retrieve seam.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import bm25_expand_oracle as orc
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import (EXC_PHRASE, EXC_TERM, EXCLUDED, FUZZY1, FUZZY2, OPTIONAL, PREFIX, REQ_PHRASE, REQ_TERM,
                                  REQUIRED, Bm25Index, QuerySyntaxError, parse_query)
from cadence_rag_amd.config import Settings

R, X, P, XP = REQ_TERM, EXC_TERM, REQ_PHRASE, EXC_PHRASE
O, Q, E = OPTIONAL, REQUIRED, EXCLUDED

# query -> (clauses, bag, text, expansions) with expand=True
PARSER_TABLE = [
    ("deploy*", [], [], "deploy", [(O, PREFIX, "deploy")]),
    ("+deploy*", [], [], "deploy", [(Q, PREFIX, "deploy")]),
    ("-deploy*", [], [], "", [(E, PREFIX, "deploy")]),
    ("kubernets~", [], [], "kubernets", [(O, FUZZY1, "kubernets")]),
    ("+kubernets~", [], [], "kubernets", [(Q, FUZZY1, "kubernets")]),
    ("-kubernets~", [], [], "", [(E, FUZZY1, "kubernets")]),
    ("kubernets~1 +Kubernets~1 -kubernets~1", [], [], "kubernets Kubernets",
     [(O, FUZZY1, "kubernets"), (Q, FUZZY1, "kubernets"), (E, FUZZY1, "kubernets")]),
    ("kubernets~2 +kubernets~2 -kubernets~2", [], [], "kubernets kubernets",
     [(O, FUZZY2, "kubernets"), (Q, FUZZY2, "kubernets"), (E, FUZZY2, "kubernets")]),
    ("(a OR b)*", [], ["a", "or"], "(a OR b)", [(O, PREFIX, "b")]),          # the item is `b)*`
    ("~2", [], ["2"], "~2", []),                                             # an operator behind zero tokens is text
    ("* ~ ~1 +* -~", [], ["1"], "~1", []),                                   # (an item without tokens is dropped)
    ("foo-bar*", [], ["foo", "bar"], "foo-bar*", []),                        # ... and behind two
    ("+foo-bar~2", [(R, ("foo",)), (R, ("bar",)), (R, ("2",))], ["foo", "bar", "2"], "foo-bar~2", []),
    ('"deploy*" "a b~2" -"x~"', [(R, ("deploy",)), (P, ("a", "b", "2")), (X, ("x",))], ["deploy", "a", "b", "2"],
     "deploy* a b~2", []),                                                   # nothing inside quotes is syntax
    ("x~3 x~0 x~12", [], ["x", "3", "x", "0", "x", "12"], "x~3 x~0 x~12", []),
    ("x** y~~ z*~", [], [], "x* y~ z*", [(O, PREFIX, "x"), (O, FUZZY1, "y"), (O, FUZZY1, "z")]),
    ('dep*"q r"', [(P, ("q", "r"))], ["q", "r"], "dep q r", [(O, PREFIX, "dep")]),   # a quote ends the item
    ("+timeout -staging dep* plain", [(R, ("timeout",)), (X, ("staging",))], ["timeout", "plain"], "timeout dep plain",
     [(O, PREFIX, "dep")]),
    ("Größ* +東京~ -ДОБРЫ~2", [], [], "Größ 東京", [(O, PREFIX, "größ"), (Q, FUZZY1, "東京"), (E, FUZZY2, "добры")]),
    ("b" * 256 + "* ok*", [], [], "ok", [(O, PREFIX, "ok")]),                # an overlong token is no token
    ("field:val* c~2", [], ["field", "val"], "field:val* c", [(O, FUZZY2, "c")]),
    ("", [], [], "", []),
    (None, [], [], "", []),
]


@pytest.mark.parametrize("case", PARSER_TABLE, ids=[repr(c[0])[:40] for c in PARSER_TABLE])
def test_parser_table(case):
    text, clauses, bag, kept, expansions = case
    got = parse_query(text, expand=True)
    assert (list(got.clauses), list(got.bag), got.text, list(got.expansions)) == (clauses, bag, kept, expansions)
    want = orc.read(text)                                                    # the oracle reads the same
    assert (list(got.clauses), list(got.bag), got.text, list(got.expansions)) == (want[0], want[1], want[2], want[3])
    # without `expand` the reading is today's: no expanding item, every operator separates tokens
    plain, old = parse_query(text), orc.read(text, expand=False)
    assert plain == parse_query(text, expand=False) and plain.expansions == ()
    assert (list(plain.clauses), list(plain.bag), plain.text) == (old[0], old[1], old[2])


def test_parser_limits():
    eight = " ".join(f"t{i}*" for i in range(8))
    assert len(parse_query(eight, expand=True).expansions) == 8
    with pytest.raises(QuerySyntaxError):
        parse_query(eight + " t8~", expand=True)
    assert len(parse_query(eight + " t8~").bag) == 9                         # not a limit without `expand`
    # required and excluded expanding items count towards the 16 constraint clauses; optional ones do not
    plain = " ".join(f"+p{i}" for i in range(12))
    ok = parse_query(plain + " +a* -b~ +c~2 -d* e* f~", expand=True)
    assert len(ok.clauses) == 12 and len(ok.expansions) == 6
    with pytest.raises(QuerySyntaxError):
        parse_query(plain + " +a* -b~ +c~2 -d* +e*", expand=True)            # 12 + 5
    with pytest.raises(QuerySyntaxError):
        parse_query("+a* -b~ +c~2 -d* " + plain + " +p12", expand=True)      # 4 + 13, the plain clause comes last
    with pytest.raises(orc.TooMuch):
        orc.read(eight + " t8~")
    with pytest.raises(orc.TooMuch):
        orc.read(plain + " +a* -b~ +c~2 -d* +e*")


# ---- the matching rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", orc.GOLDENS, ids=[f"{g[0]}-{g[1][:8]}-{g[2][:8]}" for g in orc.GOLDENS])
def test_goldens_of_the_matching_rule(case):
    kind, pattern, term, want = case
    assert orc.distance(kind, pattern, term) == want
    assert len(pattern.encode("utf-8")) <= 255 and len(term.encode("utf-8")) <= 255


def test_golden_byte_lengths_are_what_they_claim():
    assert len("caf東".encode()) - len("cafe".encode()) == 2 and orc.distance(FUZZY1, "caf東", "cafe") == 1
    assert [len(c.encode()) for c in "aï東\U00010437"] == [1, 2, 3, 4]
    assert len(orc.LONG.encode()) == 255


def test_kept_order_and_cap():
    terms = [f"ab{i:03d}" for i in range(70)] + ["ab", "abx", "xb"]
    df = np.arange(len(terms)) % 7
    ids, dist, total = orc.matches(terms, df, PREFIX, "ab")
    assert total == 72 and len(ids) == 64 and set(dist) == {0}
    assert ids == sorted(range(72), key=lambda t: (-df[t], t))[:64]          # df descending, then term id ascending
    ids, dist, total = orc.matches(terms, df, FUZZY1, "ab")
    assert (df[71], df[72]) == (1, 2) and (ids, dist, total) == ([70, 72, 71], [0, 1, 1], 3)   # distance first, then df


# ---- the weight rule ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_index(monkeypatch):
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)

    def make(texts):
        ix = Bm25Index(texts, list(range(len(texts))), "cpu")
        ix.n, ix.df = len(texts), np.diff(ix.host_csr()[0])
        return ix
    return make


def test_weight_rule(host_index):
    ix = host_index(["deploy deploy deployed", "deploy deploys", "deployed x", "deplyo", "x y", "y", "y z", "y"])
    v, n = ix.vocab, 8.0
    df = {t: int(ix.df[v[t]]) for t in v}
    assert (df["deploy"], df["deployed"], df["deploys"], df["deplyo"], df["y"]) == (2, 2, 1, 1, 4)

    def idf(d):
        return math.log(1.0 + (n - d + 0.5) / (d + 0.5)) * 2.2

    def run(query, matched):
        parsed = parse_query(query, expand=True)
        exp = [(np.asarray([v[t] for t, _ in m], dtype=np.int32), np.asarray([d for _, d in m], dtype=np.int32), len(m))
               for m in matched]
        q_ptr, terms, w = ix.expanded_terms([parsed], exp)
        assert q_ptr.tolist() == [0, len(terms)] and terms.dtype == np.int32 and w.dtype == np.float32
        assert terms.tolist() == sorted(terms.tolist())
        return dict(zip(terms.tolist(), w.tolist()))
    pre = [("deploy", 0), ("deployed", 0), ("deploys", 0)]
    fz = [("deploy", 0), ("deploys", 1), ("deployed", 2), ("deplyo", 2)]
    # a term reached by the plain bag (twice: one product) and by two items, in item order
    got = run("deploy deploy* deploy deploy~2", [pre, fz])
    base = idf(2)                                                            # df* = 2 in both items
    assert got[v["deploy"]] == float(np.float32(2.0 * math.log(1.0 + (n - 2 + 0.5) / 2.5) * 2.2 + base + base))
    assert got[v["deploys"]] == float(np.float32(base + base * 0.5))
    assert got[v["deployed"]] == float(np.float32(base + base * 0.25))
    assert got[v["deplyo"]] == float(np.float32(base * 0.25)) and len(got) == 4
    # a duplicate item counts twice
    once, twice = run("deploy*", [pre]), run("deploy* deploy*", [pre, pre])
    assert all(twice[t] == float(np.float32(2.0 * idf(2))) and once[t] == float(np.float32(idf(2))) for t in once)
    # df* is taken from a distance-2 match
    got = run("yy~2", [[("y", 1), ("x", 2)]])                                # (as if "x" had matched at distance 2)
    assert got == {v["y"]: float(np.float32(idf(4) * 0.5)), v["x"]: float(np.float32(idf(4) * 0.25))}
    got = run("zz~2", [[("z", 1), ("y", 2)]])
    assert got == {v["z"]: float(np.float32(idf(4) * 0.5)), v["y"]: float(np.float32(idf(4) * 0.25))}
    # excluded items and items without a match score nothing; the oracle gives the same weights
    got = run("-deploy* nosuch~ y", [pre, []])
    assert got == {v["y"]: float(np.float32(idf(4)))}
    ids, w = orc.weights(8, ix.df, [v["deploy"], v["deploy"]], [([v[t] for t, _ in pre], [0, 0, 0]),
                                                               ([v[t] for t, _ in fz], [d for _, d in fz])])
    want = run("deploy deploy* deploy deploy~2", [pre, fz])
    assert ids.tolist() == sorted(want) and [float(x) for x in w] == [want[t] for t in sorted(want)]


def test_group_arrays(host_index):
    parsed = [parse_query("+a* -b~ c~2 -d*", expand=True), parse_query("plain"), parse_query("+e*", expand=True)]
    i32 = lambda *x: np.asarray(x, dtype=np.int32)                           # noqa: E731
    exp = [(i32(3, 1), i32(0, 0), 2), (i32(7), i32(1), 1), (i32(9), i32(2), 1), (i32(), i32(), 0), (i32(), i32(), 0)]
    g_ptr, g_kind, gt_ptr, gt_terms = Bm25Index.group_arrays(parsed, exp)
    assert all(a.dtype == np.int32 for a in (g_ptr, g_kind, gt_ptr, gt_terms))
    # the optional item is no group, the excluded item without a match is dropped, the required one stays (empty)
    assert (g_ptr.tolist(), g_kind.tolist(), gt_ptr.tolist(), gt_terms.tolist()) == ([0, 2, 2, 3], [0, 1, 0], [0, 2, 3, 3],
                                                                                    [3, 1, 7])


def test_term_strings(host_index, monkeypatch):
    ix = host_index(["b a", "c a"])
    assert ix.term_strings() == ["b", "a", "c"]
    monkeypatch.setattr(Bm25Index, "_upload", lambda self: None)
    dec = Bm25Index.from_arrays([0, 1], [2], [1], 12, [5], "cpu")
    assert dec.term_strings() == [str(i) for i in range(12)]
    named = Bm25Index.from_arrays([0, 1], [1], [1], 2, [5], "cpu", vocab={"x": 1, "y": 0})
    assert named.term_strings() == ["y", "x"]


def test_the_oracles_group_mask():
    rows = {0: [1, 0, 1, 0, 0], 1: [0, 1, 1, 0, 0], 2: [0, 0, 0, 0, 1]}
    holds = lambda t: np.asarray(rows[t], dtype=bool)                        # noqa: E731
    assert orc.group_mask(holds, [(0, [0, 1])]).tolist() == [True, True, True, False, False]
    assert orc.group_mask(holds, [(0, [0, 1]), (1, [1, 2])]).tolist() == [True, False, False, False, False]
    assert orc.group_mask(holds, [(0, [])]).tolist() == [False] * 5 and orc.group_mask(holds, [(1, [])]).all()
    assert orc.group_mask(holds, [(0, [2]), (1, [2])]).tolist() == [False] * 5
    assert orc.group_mask(holds, [(1, [0])], [True, True, False, True, False]).tolist() == [False, True, False, True, False]
    assert orc.group_mask(holds, [], [True, False, True, False, True]).tolist() == [True, False, True, False, True]


# ---- settings and the retrieve seam ------------------------------------------------------------------------------------
def test_setting_defaults_off(monkeypatch):
    assert Settings().bm25_query_expand is False
    monkeypatch.setenv("BM25_QUERY_EXPAND", "1")
    assert Settings.from_env().bm25_query_expand is True and Settings.from_env().bm25_query_syntax is False


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

    def _rows(self, how, query_texts, k, kw):
        self.calls.append((how, list(query_texts), kw))
        ids = np.full((1, k), -1, dtype=np.int64)
        sc = np.full((1, k), np.nan, dtype=np.float32)
        ids[0, :1], sc[0, :1] = [101], [1.0]
        return ids, sc, np.array([1], dtype=np.int32)

    def search(self, query_texts, k, row_mask=None, mask_stride=0, stream=0, **kw):
        return self._rows("search", query_texts, k, kw)

    def search_query(self, query_texts, k, row_mask=None, mask_stride=0, stream=0, **kw):
        return self._rows("search_query", query_texts, k, kw)


def test_backend_passes_expand_only_when_both_settings_are_on(monkeypatch):
    word, gram = _StubLane(), _StubLane()
    be = rt.GpuRetrieveBackend(_StubTable(), _StubTable(), bm25_chunks=word, ngram_chunks=gram)
    query = "+timeout dep* -kubernets~ plain"

    def ask(syntax, expand):
        monkeypatch.setattr(rt.settings, "bm25_query_syntax", syntax)
        monkeypatch.setattr(rt.settings, "bm25_query_expand", expand)
        word.calls.clear(); gram.calls.clear()
        assert [r["chunk_id"] for r in be.fetch_chunks_bm25(query, None, None, 10)] == [101]
        assert [r["chunk_id"] for r in be.fetch_chunks_ngram(query, None, None, 10)] == [101]
        return word.calls, gram.calls
    assert ask(False, False) == ([("search", [query], {})], [("search", [query], {})])
    assert ask(False, True) == ([("search", [query], {})], [("search", [query], {})])           # not without the syntax
    assert ask(True, False) == ([("search_query", [query], {})], [("search", ["timeout dep* plain"], {})])
    # on: the word lane is told to expand, the trigram lane is given the items' text without operators
    assert ask(True, True) == ([("search_query", [query], {"expand": True})], [("search", ["timeout dep plain"], {})])
    # nine expanding items are over the limit: the bag reading on every lane
    over = " ".join(f"t{i}*" for i in range(9))
    query = over
    assert ask(True, True) == ([("search", [over], {})], [("search", [over], {})])
    assert ask(True, False) == ([("search_query", [over], {})], [("search", [over], {})])


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def call_expand(lib, fake, **kw):
    a = dict(term_ptr=fake, term_bytes=fake, post_ptr=fake, v=10, pat_ptr=_i32(0, 2, 3), pat_bytes=b"abc", pat_kind=_i32(0, 2),
             np=2, slot=fake, scratch=fake, scratch_bytes=1 << 20, terms=fake, dist=fake, kept=fake, total=fake, stream=None)
    a.update(kw)
    return lib.crag_bm25_expand_host(a["term_ptr"], a["term_bytes"], a["post_ptr"], a["v"], a["pat_ptr"], a["pat_bytes"],
                                     a["pat_kind"], a["np"], a["slot"], a["scratch"], a["scratch_bytes"], a["terms"],
                                     a["dist"], a["kept"], a["total"], a["stream"])


def expand_einval_cases(fake):
    """Every refusal the header lists, as overrides of one valid call (two patterns, 10 terms)."""
    return [dict(term_ptr=None), dict(term_bytes=None), dict(post_ptr=None), dict(pat_ptr=None), dict(pat_bytes=None),
            dict(pat_kind=None), dict(slot=None), dict(scratch=None), dict(terms=None), dict(dist=None), dict(kept=None),
            dict(total=None), dict(np=-1), dict(np=513), dict(v=-1), dict(v=2 ** 31),
            dict(pat_ptr=_i32(1, 2, 3)), dict(pat_ptr=_i32(0, 3, 2)), dict(pat_ptr=_i32(0, -1, 3)),
            dict(pat_ptr=_i32(0, 0, 3)), dict(pat_ptr=_i32(0, 3, 3)),                            # an empty pattern
            dict(pat_ptr=_i32(0, 256, 257), pat_bytes=b"a" * 257),                               # one above 255 bytes
            dict(pat_kind=_i32(0, 3)), dict(pat_kind=_i32(-1, 0)),
            dict(scratch_bytes=0), dict(scratch_bytes=2 * 64 * 8 + 8 - 1), dict(scratch=fake + 4),
            dict(terms=fake + 2), dict(dist=fake + 1), dict(kept=fake + 2), dict(total=fake + 4),
            dict(term_ptr=fake + 4), dict(post_ptr=fake + 4)]


def call_groups(lib, fake, **kw):
    a = dict(post_ptr=fake, post_pos=fake, n=100, v=7, g_ptr=_i32(0, 2), g_kind=_i32(0, 1), gt_ptr=_i32(0, 2, 3),
             gt_terms=_i32(0, 1, 2), nq=1, in_mask=None, in_stride=0, slot=fake, out=fake, stride=16, stream=None)
    a.update(kw)
    return lib.crag_bm25_group_masks_host(a["post_ptr"], a["post_pos"], a["n"], a["v"], a["g_ptr"], a["g_kind"], a["gt_ptr"],
                                          a["gt_terms"], a["nq"], a["in_mask"], a["in_stride"], a["slot"], a["out"],
                                          a["stride"], a["stream"])


def groups_einval_cases(fake):
    """Every refusal the header lists, as overrides of one valid call (a required and an excluded group, n = 100)."""
    return [dict(g_ptr=None), dict(slot=None), dict(out=None), dict(post_ptr=None), dict(post_pos=None),
            dict(g_kind=None), dict(gt_ptr=None), dict(gt_terms=None),
            dict(nq=0), dict(nq=65), dict(nq=-1), dict(n=-1), dict(n=2 ** 31), dict(v=-1), dict(v=2 ** 31),
            dict(stride=8), dict(stride=18), dict(stride=-4), dict(stride=2 ** 32 + 4), dict(out=fake + 2),
            dict(in_mask=fake, in_stride=8), dict(in_mask=fake, in_stride=18), dict(in_mask=fake + 1),
            dict(g_ptr=_i32(1, 2)), dict(g_ptr=_i32(0, -1)), dict(gt_ptr=_i32(1, 2, 3)), dict(gt_ptr=_i32(0, 3, 2)),
            dict(g_kind=_i32(0, 2)), dict(g_kind=_i32(-1, 1)),
            dict(gt_terms=_i32(7, 1, 2)), dict(gt_terms=_i32(0, 1, -1)),
            dict(gt_ptr=_i32(0, 65, 66), gt_terms=_i32(*[0] * 66)),                              # a group of 65 terms
            dict(g_ptr=_i32(0, 17), g_kind=_i32(*[0] * 17), gt_ptr=_i32(*range(18)), gt_terms=_i32(*[0] * 17))]


def test_cabi_argument_errors_without_a_device(native_lib):
    fake = 0x1000   # never dereferenced: every case is refused before the first HIP call
    for bad in expand_einval_cases(fake):
        assert call_expand(native_lib, fake, **bad) == -1, bad              # CRAG_EINVAL
        assert b"bm25_expand_host" in native_lib.crag_last_error(), bad
    for bad in groups_einval_cases(fake):
        assert call_groups(native_lib, fake, **bad) == -1, bad
        assert b"bm25_group_masks_host" in native_lib.crag_last_error(), bad
    # the zero sizes: CRAG_OK, nothing enqueued
    assert call_expand(native_lib, fake, np=0, pat_ptr=None, pat_bytes=None, pat_kind=None, terms=None, dist=None, kept=None,
                       total=None, scratch=None, scratch_bytes=0, slot=None) == 0
    assert call_groups(native_lib, fake, n=0, stride=0, post_ptr=None, post_pos=None, out=None) == 0
    assert native_lib.crag_bm25_expand_scratch_bytes(0, 5) == 0
    assert native_lib.crag_bm25_expand_scratch_bytes(4097, 3) == 2 * 3 * 64 * 8 + 24
    assert native_lib.crag_bm25_expand_scratch_bytes(-1, 3) == -1 and native_lib.crag_bm25_expand_scratch_bytes(5, 513) == -1


def test_the_clause_entry_still_refuses_what_it_refused(native_lib):
    """Kind 5 and term clauses of two terms are no way into the any-of groups: the clause entry is unchanged."""
    fake = 0x1000
    lib = native_lib
    args = lambda kind, ct_ptr, terms: (fake, fake, fake, fake, 100, 7, _i32(0, 1), kind, ct_ptr, terms, 1, None, 0, fake,  # noqa: E731
                                        fake, 16, None)
    assert lib.crag_bm25_clause_masks_host(*args(_i32(5), _i32(0, 1), _i32(0))) == -1
    assert lib.crag_bm25_clause_masks_host(*args(_i32(0), _i32(0, 2), _i32(0, 1))) == -1
