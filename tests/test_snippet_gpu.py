"""Query-aware snippet windows on the GPU (crag_bm25_snippets_host) against the brute-force oracle of
snippet_oracle.py, which tries every start.  All four outputs are compared bit for bit; there is no tolerance."""
import numpy as np
import pytest

import snippet_oracle as so
from bm25_clause_oracle import arrays_from_rows
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import SNIPPET_STAGE, Bm25Index, tokenize
from cadence_rag_amd.snippets import clip

pytestmark = pytest.mark.gpu
F = 9            # a filler term no query asks for


def build(rows, n_terms):
    row_ptr, terms, tfs, pair_off, pair_where = arrays_from_rows(rows)
    return Bm25Index.from_arrays(row_ptr, terms, tfs, n_terms, np.arange(len(rows)), "cuda:0", pair_off=pair_off,
                                 pair_where=pair_where)


def run(ix, args, window):
    start, last, score, covered = ix.snippet_windows_terms(*args, window)
    return (start.cpu().numpy(), last.cpu().numpy(), score.cpu().numpy(), covered.cpu().numpy().view(np.uint64))


def check(rows, n_terms, queries, pairs, windows):
    """The GPU's four outputs == the oracle's, bit for bit, at every window; returns the last window's outputs."""
    ix = build(rows, n_terms)
    args = so.batch(queries, pairs)
    got = None
    try:
        for window in windows:
            got, want = run(ix, args, window), so.windows(rows, *args, window)
            for g, w, name in zip(got, want, ("start", "last", "score", "covered")):
                assert g.dtype == w.dtype and g.shape == w.shape, (name, window)
                same = np.array_equal(g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else np.array_equal(g, w)
                assert same, (name, window, g[:16], w[:16])
    finally:
        ix.close()
    return got


# ---- edges ------------------------------------------------------------------------------------------------------------
def test_one_term_one_occurrence_and_the_widths(gpu):
    rows = [[F] * 40 + [0] + [F] * 9]
    got = check(rows, 10, [([0], [1.5])], [[0]], [1, 2, 120, 65535])
    assert got[0].tolist() == [40] and got[1].tolist() == [40] and got[2].tolist() == [1.5] and got[3].tolist() == [1]


def test_exactly_w_apart_and_one_less(gpu):
    rows = [[0] + [F] * 9 + [1] + [F] * 5]                     # the two terms stand 10 apart
    both = check(rows, 10, [([0, 1], [1.0, 2.0])], [[0]], [11])
    assert both[0].tolist() == [0] and both[1].tolist() == [10] and both[3].tolist() == [3] and both[2].tolist() == [3.0]
    apart = check(rows, 10, [([0, 1], [1.0, 2.0])], [[0]], [10])   # W = 10: [0, 10) does not reach position 10
    assert apart[0].tolist() == [10] and apart[3].tolist() == [2] and apart[2].tolist() == [2.0]


def test_equal_scores_go_to_the_lower_start(gpu):
    rows = [[F, 0, F, 1, F, F, F, F, 1, F, 0, F, F]]            # {0, 1} inside 3 tokens at 1 and again at 8
    got = check(rows, 10, [([0, 1], [1.0, 1.0])], [[0]], [3, 4])
    assert got[0].tolist() == [1] and got[1].tolist() == [3]
    # ... also when the lanes that hold the two starts are far apart: 70 occurrences of term 0, equal windows at both ends
    rows = [[0, 1] + [F] * 5 + [0, F, F] * 68 + [F] * 5 + [0, 1]]
    got = check(rows, 10, [([0, 1], [1.0, 1.0])], [[0]], [2])
    assert got[0].tolist() == [0] and got[2].tolist() == [2.0]


def test_a_position_at_65534(gpu):
    rows = [[F] * 30000 + [0] + [F] * 35533 + [0, 1, 1], [1]]   # term 0 at 30000 and 65534; 65535 and 65536 are not indexed
    got = check(rows, 10, [([0], [1.0]), ([1], [1.0]), ([0, 1], [1.0, 4.0])], [[0], [0, 1], [0, 1]], [1, 9, 65535])
    assert got[0].tolist() == [30000, -1, 0, 30000, 0] and got[1].tolist() == [65534, 0, 0, 65534, 0]


# ---- row lookup -------------------------------------------------------------------------------------------------------
def test_row_lookup(gpu):
    # term 0: rows 0, 3, 7 (first / middle / last posting, row 0 and row n - 1); term 1: rows 2 and 4 only, the neighbours of 3;
    # term 2: every row; term 3: no row; row 5 holds none of the first two
    rows = [[0, F, 2], [F, 2, F], [1, 2], [F, F, 0, 2, F, 0], [2, 1, 1], [F, 2], [2], [2, F, F, 0]]
    n = len(rows)
    queries = [([0], [1.0]), ([0, 1], [1.0, 2.0]), ([1], [3.0]), ([3], [1.0]), ([0, 1, 3], [1.0, 1.0, 1.0]), ([0, 1, 2], [1.0, 1.0, 0.5])]
    pairs = [list(range(n)), [3, 3, 0, n - 1, 3], [3, 2, 4], list(range(n)), [5, 1, 6], list(range(n - 1, -1, -1))]
    got = check(rows, 10, queries, pairs, [1, 2, 5])
    start = got[0].tolist()
    assert start[:n] == [0, -1, -1, 2, -1, -1, -1, 3]                       # query 0 over every row
    assert start[n:n + 5] == [2, 2, 0, 3, 2]                                # a repeated row gives the same answer thrice
    assert start[n + 5:n + 8] == [-1, 0, 1]                                 # term 1 holds only the neighbours of row 3
    assert start[n + 8:2 * n + 8] == [-1] * n and start[2 * n + 8:2 * n + 11] == [-1, -1, -1]
    for out in got[1:]:
        assert not out[n + 8:2 * n + 11].any()                             # -1 comes with 0 / 0 / 0


# ---- shape ------------------------------------------------------------------------------------------------------------
def test_one_slot_and_64_slots(gpu):
    rng = np.random.default_rng(5)
    rows = [rng.integers(0, 80, size=n).tolist() for n in (700, 64, 1, 300)] + [list(range(64)), list(range(63, -1, -1))]
    weights = rng.uniform(0.25, 9.0, size=64).astype(np.float32).tolist()
    queries = [(list(range(64)), weights), ([17], [2.5]), (list(range(8, 72)), weights[::-1])]
    got = check(rows, 80, queries, [list(range(6))] * 3, [1, 7, 64, 120])
    assert got[3][4] == np.uint64(2 ** 64 - 1) and got[3][5] == np.uint64(2 ** 64 - 1)   # W = 120: every slot covered


def test_more_occurrences_than_lanes(gpu):
    rng = np.random.default_rng(6)
    rows = [rng.integers(0, 3, size=150).tolist(), [0] * 200, ([0] * 70 + [F] * 30 + [1, 0, 2]) * 2]
    check(rows, 10, [([0, 1, 2], [1.0, 2.0, 4.0]), ([0], [1.0])], [[0, 1, 2], [1, 2, 0]], [1, 3, 31, 100])


@pytest.mark.parametrize("extra", [0, 1])
def test_either_side_of_the_staging_switch(gpu, extra):
    # the pair's positions number SNIPPET_STAGE (staged in LDS) or SNIPPET_STAGE + 1 (read from memory); the best window,
    # the only place where 1 and 2 stand close together, is at the far end of the row
    n0 = SNIPPET_STAGE - 6 + extra
    rows = [[0, F, 1, F, F, F, 2, F, F] + [0] * (n0 - 1) + [F] * 9 + [1, F, 2, 1, 2]]
    got = check(rows, 10, [([0, 1, 2], [1.0, 2.0, 4.0])], [[0]], [2, 3, 7, 65535])
    assert got[3].tolist() == [7]
    assert sum(len([t for t in rows[0] if t == j]) for j in range(3)) == SNIPPET_STAGE + extra
    if extra:   # the same row with a query of two slots stays below the switch and gives the same windows for {1, 2}
        check(rows, 10, [([1, 2], [2.0, 4.0])], [[0]], [2, 3, 7])


def test_64_queries_some_without_rows_and_no_pairs_at_all(gpu):
    rng = np.random.default_rng(7)
    rows = [rng.integers(0, 12, size=60).tolist() for _ in range(30)]
    queries = [(np.sort(rng.choice(12, size=1 + q % 4, replace=False)).tolist(), [1.0 + q] * (1 + q % 4)) for q in range(64)]
    pairs = [[] if q % 3 == 0 else rng.integers(0, 30, size=q % 7).tolist() for q in range(64)]
    assert not pairs[0] and not pairs[63] and not pairs[7]
    check(rows, 12, queries, pairs, [5])
    got = check(rows, 12, queries, [[] for _ in range(64)], [5])
    assert all(out.size == 0 for out in got)
    got = check(rows, 12, [([], [])] * 2 + [([3], [1.0])], [[0, 1], [], [2]], [5])      # queries without slots
    assert got[0][:2].tolist() == [-1, -1]


# ---- the order of the sum ---------------------------------------------------------------------------------------------
def test_the_sum_runs_in_slot_order(gpu):
    rows = [[0, 1, 2]]
    big = float(2 ** 24)
    first = check(rows, 10, [([0, 1, 2], [big, 1.0, 1.0])], [[0]], [3])
    last = check(rows, 10, [([0, 1, 2], [1.0, 1.0, big])], [[0]], [3])
    assert first[2].view(np.uint32).tolist() == np.array([2 ** 24], dtype=np.float32).view(np.uint32).tolist()
    assert last[2].view(np.uint32).tolist() == np.array([2 ** 24 + 2], dtype=np.float32).view(np.uint32).tolist()


# ---- the random case --------------------------------------------------------------------------------------------------
def test_the_random_case(gpu):
    rows, queries, pairs = so.random_case()
    got = check(rows, 50, queries, pairs, [7, 120])
    assert got[0].size == 1600 and (got[0] >= 0).all()


# ---- end to end -------------------------------------------------------------------------------------------------------
TEXTS = ["The gateway returned a timeout; we retried.", "Nothing of note here, only small talk about the weather.",
         " ".join(f"pad{i}" for i in range(500)) + " then the Gateway TIMEOUT was fixed by a rollback",
         "timeout timeout timeout " + " ".join(f"x{i}" for i in range(300)) + " gateway error", ""]
IDS = [10, 11, 20, 35, 40]


def test_snippet_windows_by_ids_on_an_index_built_from_texts(gpu):
    ix = Bm25Index(TEXTS, IDS, "cuda:0", positions=True)
    try:
        queries = ["gateway timeout", '+rollback -gateway "small talk" nosuchword', "pad3 pad7"]
        lists = [[35, 10, 20, 11, 40], [20, 11], [20, 20, 10]]
        start, last, score, covered = (t.cpu().numpy() for t in ix.snippet_windows(queries, lists, 12))
        rows = [[ix.vocab[t] for t in tokenize(text)] for text in TEXTS]
        q_ptr, terms, weights = ix.snippet_terms(queries)
        r_ptr = np.array([0, 5, 7, 10], dtype=np.int32)
        pos = np.array([3, 0, 2, 1, 4, 2, 1, 2, 2, 0], dtype=np.int32)
        want = so.windows(rows, q_ptr, terms, weights, r_ptr, pos, 12)
        for g, w in zip((start, last, score.view(np.uint32), covered.view(np.uint64)),
                        (want[0], want[1], want[2].view(np.uint32), want[3])):
            assert np.array_equal(g, w)
        assert start.tolist()[:5] == [0, 1, 502, -1, -1] and start.tolist()[5:7] == [508, 5]
        with pytest.raises(ValueError, match="does not hold"):
            ix.snippet_windows(["gateway"], [[10, 12]], 12)
        with pytest.raises(ValueError, match="does not hold"):
            ix.snippet_windows(["gateway"], [[41]], 12)
    finally:
        ix.close()
    plain = Bm25Index(TEXTS, IDS, "cuda:0")
    try:
        with pytest.raises(ValueError, match="positions"):
            plain.snippet_windows(["gateway"], [[10]], 12)
    finally:
        plain.close()


def test_retrieve_evidence_cuts_the_snippet_where_the_query_word_is(gpu, monkeypatch):
    from datetime import datetime
    from uuid import UUID

    from helpers import unit_rows
    rng = np.random.default_rng(8)
    call = {"call_id": UUID(int=1), "external_id": "ext", "external_source": "zoom"}
    filler = " ".join(f"filler{i}" for i in range(400))           # about 3 600 characters
    texts = [filler + " and then the rollback happened " + filler[:200], "rollback first. " + filler, filler]

    def make(name, id_field, body, rows, extra):
        n = len(rows)
        cols = {id_field: [100 + i for i in range(n)], "call_id": [call["call_id"]] * n, body: rows}
        cols.update(extra(n))
        table = rt.DenseTable(name, id_field, dim=1024, capacity=n + 64)
        table.add(unit_rows(rng, n), cols, call_started_at=[datetime(2026, 3, 1)] * n, call_tags={call["call_id"]: []})
        return table
    chunks = make("chunks", "chunk_id", "text", texts, lambda n: {
        "speaker": ["S"] * n, "start_ts_ms": [0] * n, "end_ts_ms": [9] * n})
    arts = make("artifact_chunks", "artifact_chunk_id", "content", texts[:1], lambda n: {
        "artifact_id": list(range(n)), "kind": ["summary"] * n})
    be = None
    try:
        be = rt.GpuRetrieveBackend(chunks, arts, calls=[call], bm25_chunks=chunks.build_bm25_lane("text", positions=True),
                                   bm25_artifacts=arts.build_bm25_lane("content"))     # the artifact lane: no positions
        req = rt.RetrieveRequest(query="rollback")
        strip = lambda r: {k: v for k, v in r.items() if k != "query_id"}   # noqa: E731
        monkeypatch.setattr(rt.settings, "snippet_best", False)
        asked, ask = [], be.snippet_windows
        monkeypatch.setattr(be, "snippet_windows", lambda *a: asked.append(a[:2]) or ask(*a))
        off = rt.retrieve_evidence(req, be)
        assert asked == []                                                  # the knob is off: no new call
        by_id = {q["chunk_id"]: q["snippet"] for q in off["quotes"]}
        assert by_id == {100: clip(texts[0], 800), 101: clip(texts[1], 800)} and "rollback" not in by_id[100]
        assert off["artifacts"][0]["snippet"] == clip(texts[0], 800) and "snippet_mode" not in off["notes"]["retrieval"]

        monkeypatch.setattr(rt.settings, "snippet_best", True)
        on = rt.retrieve_evidence(req, be)
        assert asked == [("artifact_chunks", "rollback"), ("chunks", "rollback")]   # one question per side
        got = {q["chunk_id"]: q["snippet"] for q in on["quotes"]}
        assert "rollback" in got[100] and got[100].startswith("…filler395 ") and len(got[100]) <= 800   # token 403 - 8
        assert got[101] == by_id[101]                                       # the word stands in front: the head clip
        assert on["artifacts"][0]["snippet"] == clip(texts[0], 800)         # a lane without positions: the head clip
        assert on["notes"]["retrieval"].pop("snippet_mode") == "best"
        for q in on["quotes"]:
            q["snippet"] = by_id[q["chunk_id"]]
        assert strip(on) == strip(off)                                      # nothing else moved
    finally:
        if be is not None:
            for lane in be._bm25.values():
                lane.close()
        chunks.close()
        arts.close()
