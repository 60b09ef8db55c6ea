"""Prefix and fuzzy items of the BM25 lane on the GPU: crag_bm25_expand_host and
crag_bm25_group_masks_host against the oracle written from the header's prose (tests/bm25_expand_oracle.py), and
Bm25Index.search_query(expand=True), retrieve_evidence and HybridSearcher against the fp32 replay (tests/bm25_replay.py)
under the oracle's mask and weights.  Every comparison is exact: ids, distances, counts, mask bytes, score bits."""
import ctypes

import numpy as np
import pytest
import torch

import bm25_expand_oracle as orc
from bm25_clause_oracle import ClauseOracle, packed
from bm25_replay import NAN_BITS, assert_equals_replay, replay_index
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import (BM25_EXPAND_SLICE, FUZZY1, FUZZY2, MAX_EXPANSIONS, PREFIX, RANGE_ROWS, Bm25Index,
                                  tokenize)
from cadence_rag_amd.dense_index import DenseIndex
from test_bm25_syntax_gpu import text_corpus

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S = BM25_EXPAND_SLICE


def planted_index(terms, df):
    """An index whose term t is terms[t] and is held by the rows 0 .. df[t] - 1."""
    df = np.asarray(df, dtype=np.int64)
    n = max(int(df.max()), 1)
    per_row = [np.flatnonzero(df > r).astype(np.int32) for r in range(n)]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([r.size for r in per_row], out=row_ptr[1:])
    row_terms = np.concatenate(per_row)
    ix = Bm25Index.from_arrays(row_ptr, row_terms, np.ones(row_terms.size, dtype=np.int64), len(terms),
                               np.arange(n, dtype=np.int64), DEV, vocab={t: i for i, t in enumerate(terms)})
    assert np.array_equal(ix.df, df)
    return ix


def vocabulary(v):
    """v terms that all begin with "w": numbered fillers, and at the edges of the slices the words the patterns look for;
    families of 63, 64 and 65 terms inside one slice and spread over three.  df in 0 .. 3, so that ties are everywhere."""
    terms = [f"w{i:05d}" for i in range(v)]
    plant = {0: "wdeploy", S - 1: "wdeployed", S: "wdeploys", 2 * S - 1: "wdeplox", 2 * S: "wdepoly", v - 1: "wdeployment"}
    for k in (63, 64, 65):
        for j in range(k):
            plant[100 * (k - 62) + j] = f"wfam{k}a{j:02d}"                          # inside the first slice
            plant[(j % 3) * S + 1000 + 100 * (k - 63) + j] = f"wfam{k}b{j:02d}"     # over three slices
    for at, name in plant.items():
        if at < v:
            terms[at] = name
    assert len(set(terms)) == v
    return terms, (np.arange(v) * 7919) % 4


BASE_PATTERNS = [(PREFIX, "wdeploy"), (FUZZY1, "wdeploy"), (FUZZY2, "wdeploy"), (FUZZY2, "wdeployd"), (PREFIX, "w"),
                 (PREFIX, "w0000"), (FUZZY1, "w00000"), (FUZZY2, "w00000"), (FUZZY2, "w04095"), (PREFIX, "zzz"),
                 (FUZZY2, "qqqqqqqq"), (PREFIX, "wfam63a"), (PREFIX, "wfam64a"), (PREFIX, "wfam65a"), (PREFIX, "wfam63b"),
                 (PREFIX, "wfam64b"), (PREFIX, "wfam65b"), (FUZZY1, "wfam65b00"), (FUZZY2, "wfam64a63"), (PREFIX, "wdeployment"),
                 (FUZZY1, "wdeploymen"), (PREFIX, "wdeploymentx"), (FUZZY1, "w"), (FUZZY2, "w")]
_want = {}


def check_expand(ix, terms, patterns, key):
    got = ix.expand(patterns)
    assert len(got) == len(patterns)
    for (kind, pat), (ids, dist, total) in zip(patterns, got):
        if (key, kind, pat) not in _want:
            _want[key, kind, pat] = orc.matches(terms, ix.df, kind, pat)
        want = _want[key, kind, pat]
        assert ids.dtype == np.int32 and dist.dtype == np.int32
        assert (ids.tolist(), dist.tolist(), total) == want, (kind, pat, len(terms))
    return got


@pytest.fixture(scope="module")
def big(gpu):
    terms, df = vocabulary(3 * S - 7)      # three slices, the last one short
    ix = planted_index(terms, df)
    yield ix, terms
    ix.close()


@pytest.mark.parametrize("v", [1, S - 1, S, S + 1, 2 * S + 3])
def test_expand_at_the_slice_edges(gpu, v):
    terms, df = vocabulary(v)
    ix = planted_index(terms, df)
    try:
        got = check_expand(ix, terms, BASE_PATTERNS, v)
        assert got[4][2] == v and len(got[4][0]) == min(v, MAX_EXPANSIONS)      # `w*` matches every term
        assert got[9][0].size == 0 and got[9][2] == 0                            # `zzz*`: no match
    finally:
        ix.close()


def test_expand_over_three_slices(big):
    ix, terms = big
    v = len(terms)
    got = dict(zip(BASE_PATTERNS, check_expand(ix, terms, BASE_PATTERNS, v)))
    t = {name: i for i, name in enumerate(terms)}
    # matches at the first and last term of a slice and at the last term of the vocabulary
    assert set(got[PREFIX, "wdeploy"][0].tolist()) == {0, S - 1, S, v - 1}
    assert set(got[FUZZY2, "wdeploy"][0].tolist()) == {0, S, 2 * S - 1, 2 * S, S - 1}
    assert got[FUZZY1, "wdeploymen"][0].tolist() == [v - 1] and got[PREFIX, "wdeploymentx"][2] == 0
    for k in (63, 64, 65):
        for fam in "ab":
            ids, dist, total = got[PREFIX, f"wfam{k}{fam}"]
            assert total == k and len(ids) == min(k, 64) and not dist.any()
            members = [t[f"wfam{k}{fam}{j:02d}"] for j in range(k)]
            assert ids.tolist() == sorted(members, key=lambda i: (-ix.df[i], i))[:64]   # ties on df by term id, across slices
    assert got[PREFIX, "w"][2] == v and got[PREFIX, "w"][0].size == 64
    assert got[PREFIX, "zzz"][2] == 0 and got[FUZZY2, "qqqqqqqq"][2] == 0
    assert got[FUZZY2, "w00000"][2] > 64                                         # the cap cuts inside a distance class


def test_512_patterns_in_one_call_and_alone(big):
    ix, terms = big
    more = []
    for i in range(512 - len(BASE_PATTERNS)):
        if i % 50 == 7:
            more.append((1 + i % 2, f"w{i * 16:05d}"[:5] + "x"))                 # one code point off a filler
        elif i % 3 == 0:
            more.append((PREFIX, f"w{i % 82:02d}"))
        else:
            more.append((1 + i % 2, f"w{i:05d}zzzzzzzz"))                        # longer than every term
    batch = BASE_PATTERNS + more
    assert len(batch) == 512
    got = check_expand(ix, terms, batch, len(terms))
    for at in (0, 2, 7, 14, 30, 511):                                            # the same pattern alone: the same output
        alone = ix.expand([batch[at]])[0]
        assert alone[0].tolist() == got[at][0].tolist() and alone[1].tolist() == got[at][1].tolist() and alone[2] == got[at][2]
    with pytest.raises(ValueError):
        ix.expand(batch + [(PREFIX, "w")])


def test_more_matching_slices_than_the_merge_holds_in_lds(gpu):
    """65 slices that all match: 65 * 64 keys reach the merge, one more than it compacts into LDS."""
    v = 65 * S + 1
    terms = [f"w{i:06d}" for i in range(v)]
    ix = planted_index(terms, (np.arange(v) * 7919) % 4)
    try:
        got = check_expand(ix, terms, [(PREFIX, "w"), (PREFIX, "w26624"), (PREFIX, "w0000")], v)
        assert got[0][2] == v and got[0][0].size == 64 and got[1][0].tolist() == [v - 1] and got[2][2] == 100
    finally:
        ix.close()


def test_the_goldens_on_the_device(gpu):
    terms = sorted({g[2] for g in orc.GOLDENS}) + [f"pad{i}" for i in range(40)]
    ix = planted_index(terms, (np.arange(len(terms)) * 5) % 3 + 1)
    try:
        patterns = sorted({(g[0], g[1]) for g in orc.GOLDENS})
        got = dict(zip(patterns, check_expand(ix, terms, patterns, "goldens")))
        for kind, pat, term, want in orc.GOLDENS:
            ids, dist, _ = got[kind, pat]
            found = dict(zip(ids.tolist(), dist.tolist())).get(terms.index(term))
            assert found == want, (kind, pat, term)
    finally:
        ix.close()


def test_the_decimal_vocabulary_and_extend(gpu):
    dec = Bm25Index.from_arrays([0, 1, 2], [3, 120], [1, 1], 130, [5, 9], DEV)
    try:
        names = [str(i) for i in range(130)]
        check_expand(dec, names, [(PREFIX, "12"), (FUZZY1, "12"), (FUZZY2, "120"), (PREFIX, "3")], "decimal")
    finally:
        dec.close()
    texts = text_corpus(120) + ["deployment deployed conection", "deploys the gatewya"]
    grown = Bm25Index(texts[:70], np.arange(70), DEV)
    fresh = Bm25Index(texts, np.arange(len(texts)), DEV)
    try:
        patterns = [(PREFIX, "deploy"), (FUZZY1, "conection"), (FUZZY2, "gateway"), (PREFIX, "re")]
        before = grown.expand(patterns)                                           # (uploads the dictionary of 70 rows)
        grown.extend(texts[70:], np.arange(70, len(texts)))
        a, b = grown.expand(patterns), fresh.expand(patterns)
        for x, y in zip(a, b):
            assert x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() and x[2] == y[2]
        assert a[0][2] == 4 and before[0][2] == 1
        check_expand(fresh, fresh.term_strings(), patterns, "text")
    finally:
        grown.close(); fresh.close()


# ---- group masks -------------------------------------------------------------------------------------------------------
def _i32(values):
    return np.ascontiguousarray(values, dtype=np.int32)


def run_group_masks(ix, groups_per_query, in_mask, stride, guard=64):
    """The entry on a poisoned buffer -> (the nq runs' bytes, the guard bytes behind them)."""
    nq = len(groups_per_query)
    g_ptr, kinds, gt_ptr, gt_terms = [0], [], [0], []
    for groups in groups_per_query:
        for kind, ids in groups:
            kinds.append(kind)
            gt_terms.extend(ids)
            gt_ptr.append(len(gt_terms))
        g_ptr.append(len(kinds))
    g_ptr, kinds, gt_ptr, gt_terms = _i32(g_ptr), _i32(kinds), _i32(gt_ptr), _i32(gt_terms)
    out = torch.full((nq * stride + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    d_in = in_stride = None
    if in_mask is not None:
        pk = DenseIndex.pack_mask(np.asarray(in_mask))
        d_in, in_stride = torch.from_numpy(pk).to(DEV), (pk.shape[-1] if pk.ndim == 2 else 0)
    from cadence_rag_amd import _native
    rc = _native.load().crag_bm25_group_masks_host(
        ix.d_post_ptr.data_ptr(), ix.d_post_pos.data_ptr(), ix.n, ix.n_terms, g_ptr.ctypes.data,
        kinds.ctypes.data if kinds.size else None, gt_ptr.ctypes.data, gt_terms.ctypes.data if gt_terms.size else None, nq,
        None if d_in is None else d_in.data_ptr(), in_stride or 0, ix._slot(0), out.data_ptr(), stride, ctypes.c_void_p(0))
    _native.check(rc, "crag_bm25_group_masks_host")
    host = out.cpu().numpy()
    return host[:nq * stride], host[nq * stride:]


def run_clause_masks(ix, clauses_per_query, in_mask, stride):
    """crag_bm25_clause_masks_host for term clauses (kind, term id) -> the runs' bytes."""
    nq = len(clauses_per_query)
    c_ptr = _i32(np.concatenate([[0], np.cumsum([len(c) for c in clauses_per_query])]))
    flat = [c for cs in clauses_per_query for c in cs]
    c_kind, ct_ptr, ct_terms = _i32([k for k, _ in flat]), _i32(np.arange(len(flat) + 1)), _i32([t for _, t in flat])
    out = torch.full((nq * stride,), 0xCD, dtype=torch.uint8, device=DEV)
    d_in = in_stride = None
    if in_mask is not None:
        pk = DenseIndex.pack_mask(np.asarray(in_mask))
        d_in, in_stride = torch.from_numpy(pk).to(DEV), (pk.shape[-1] if pk.ndim == 2 else 0)
    ix._clause_launch(c_ptr, c_kind, ct_ptr, ct_terms, nq, d_in, in_stride or 0, out, stride, 0)
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 31, 32, 33, RANGE_ROWS - 1, RANGE_ROWS, RANGE_ROWS + 1, 2 * RANGE_ROWS + 5])
def test_group_masks_against_the_oracle(gpu, n):
    rng = np.random.default_rng(n)
    v = 96
    p = 1.0 / np.arange(1, v + 1) ** 1.3
    lens = rng.integers(0, 7, size=n)
    flat = rng.choice(v, size=int(lens.sum()), p=p / p.sum())
    rows = [np.unique(r) for r in np.split(flat, np.cumsum(lens)[:-1])]
    rows[-1] = np.unique(np.append(rows[-1], [0, 95]))                           # the last row holds a common and a rare term
    row_ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    row_terms = np.concatenate(rows).astype(np.int32)
    ix = Bm25Index.from_arrays(row_ptr, row_terms, np.ones(row_terms.size, dtype=np.int64), v, np.arange(n), DEV)
    try:
        clause_oracle = ClauseOracle(rows)
        holds = clause_oracle.holds_term
        every = list(range(16, 80))
        queries = [[(0, [3])], [(1, [0])],                                        # one term: the clause entry's output
                   [(0, every)], [(1, every)],                                    # 64 terms
                   [(g % 2, [int(x) for x in rng.choice(v, size=1 + g * 4, replace=False)]) for g in range(16)],
                   [(0, [0, 1, 2]), (1, [2, 5])],                                 # a term in a required and an excluded group
                   [(0, [])], [(1, [])], [(1, []), (0, [1, 4])], [(0, [0, 1]), (0, [])],
                   [], [(0, [95, 0])]]
        nq = len(queries)
        min_stride = (n + 31) // 32 * 4
        for in_mask in (None, rng.random(n) < 0.7, rng.random((nq, n)) < 0.7):
            for stride in (min_stride, min_stride + 8):
                want = np.stack([orc.group_mask(holds, groups, None if in_mask is None else
                                                (in_mask[q] if np.ndim(in_mask) == 2 else in_mask))
                                 if groups or in_mask is not None else np.ones(n, dtype=bool)
                                 for q, groups in enumerate(queries)])
                runs, guard = run_group_masks(ix, queries, in_mask, stride)
                assert np.array_equal(runs, packed(want, stride)), (n, stride)    # every byte written, the padding zero
                assert np.all(guard == 0xAB)                                      # ... and nothing behind the runs
            term_clauses = [[(0, 3)], [(1, 0)]]
            im = None if in_mask is None else (in_mask[:2] if np.ndim(in_mask) == 2 else in_mask)
            runs, _ = run_group_masks(ix, queries[:2], im, min_stride)
            assert np.array_equal(runs, run_clause_masks(ix, term_clauses, im, min_stride))
    finally:
        ix.close()


# ---- end to end --------------------------------------------------------------------------------------------------------
VARIANTS = ["deployment", "deployed", "deploys", "conection", "connexion", "timeouts", "gatewya", "retries", "redeploy"]
QUERIES = ["deploy*", "+deploy* error", "-deploy* error retry", "conection~", "+conection~ reset", "connextion~2 -staging",
           'timeout* "connection reset"', "+gatewya~2 -the", "nosuch* error", "+nosuch~ error", "-nosuch~2 error",
           "deploy deploy* deploy deploy~2", 're* +"we saw"', "plain words only error", "+time* -timeouts*",
           "+re* +de* -conn* the", "-the~ a~2 we~", "retry~2 +gateway* -prod~", "(staging OR prod)* error",
           "deploy* deploy*"]


def expand_corpus(n=200):
    texts = text_corpus(n)
    rng = np.random.default_rng(4)
    for i in rng.choice(n, size=60, replace=False):
        texts[i] += " " + " ".join(rng.choice(VARIANTS, size=int(rng.integers(1, 3))))
    return texts


def predict(ix, clause_oracle, terms, queries, k, eligible=None):
    """What the rule says the lane returns: the replay under the oracle's mask with the oracle's weights."""
    q_ptr, ids, ws, masks = [0], [], [], []
    for q, text in enumerate(queries):
        clauses, groups, t, w = orc.query_plan(text, terms, ix.df, ix.n, ix.vocab.get)
        el = None if eligible is None else (eligible[q] if np.ndim(eligible) == 2 else eligible)
        masks.append(orc.group_mask(clause_oracle.holds_term, groups, clause_oracle.passes(clauses, el)))
        ids.extend(t.tolist()); ws.extend(w.tolist())
        q_ptr.append(len(ids))
    return replay_index(ix, np.asarray(q_ptr, dtype=np.int32), np.asarray(ids, dtype=np.int32),
                        np.asarray(ws, dtype=np.float32), k, np.stack(masks))


@pytest.fixture(scope="module")
def text_index(gpu):
    texts = expand_corpus()
    ix = Bm25Index(texts, np.arange(len(texts), dtype=np.int64) * 2 + 500, DEV, positions=True)
    yield ix, ClauseOracle([[ix.vocab[t] for t in tokenize(text)] for text in texts]), ix.term_strings()
    ix.close()


@pytest.mark.parametrize("k", [1, 10, 128])
def test_search_query_with_expand_equals_the_replay_under_the_oracle(text_index, k):
    ix, clause_oracle, terms = text_index
    rng = np.random.default_rng(k)
    for eligible in (None, rng.random(len(ix)) < 0.6, rng.random((len(QUERIES), len(ix))) < 0.6):
        mask, stride = None, 0
        if eligible is not None:
            pk = DenseIndex.pack_mask(eligible)
            mask, stride = torch.from_numpy(pk).to(DEV), (pk.shape[-1] if pk.ndim == 2 else 0)
        ids, sc, ct = [x.cpu().numpy() for x in ix.search_query(QUERIES, k, row_mask=mask, mask_stride=stride, expand=True)]
        print(f"k={k} filter={'none' if eligible is None else np.ndim(eligible)}: counts {ct.tolist()}")
        assert_equals_replay(predict(ix, clause_oracle, terms, QUERIES, k, eligible), ids, sc, ct, f"k={k}")
        assert np.all(sc.view(np.uint32)[ids < 0] == NAN_BITS)
        if eligible is None:
            assert (ct > 0).sum() >= len(QUERIES) // 2 and ct[QUERIES.index("+nosuch~ error")] == 0
    one = [x.cpu().numpy() for x in ix.search_query(QUERIES[3:4], k, expand=True)]      # alone as in the batch
    assert_equals_replay(predict(ix, clause_oracle, terms, QUERIES[3:4], k), *one, "alone")
    # without `expand` the operators are text, as they were
    plain = [x.cpu().numpy() for x in ix.search_query(QUERIES[:4], k)]
    want = [x.cpu().numpy() for x in ix.search_query([q.replace("*", " ").replace("~", " ") for q in QUERIES[:4]], k)]
    assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1].view(np.uint32), want[1].view(np.uint32))


def test_a_batch_without_operators_is_search(text_index, monkeypatch):
    ix, _, _ = text_index

    def no_expand(*a, **kw):
        raise AssertionError("a batch without expanding items must not reach the expand entry")
    monkeypatch.setattr(ix, "expand", no_expand)
    queries = ["connection reset", "the gateway error-retry", "nothing known here", "", "~2 foo-bar* x~3"]
    a = [x.cpu().numpy() for x in ix.search_query(queries, 20, expand=True)]
    b = [x.cpu().numpy() for x in ix.search(queries, 20)]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_retrieve_and_hybrid_with_the_settings_on_and_off(gpu, monkeypatch):
    """Lexical-only retrieve_evidence over native word lanes == the same request over a CPU composition whose BM25 rows are
    the replay's under the reading the settings select; HybridSearcher's native lane likewise."""
    from datetime import datetime, timedelta
    from uuid import UUID

    from cadence_rag_amd import embeddings
    from cadence_rag_amd.fusion import HybridSearcher
    from helpers import unit_rows
    rng = np.random.default_rng(22)
    texts = expand_corpus()
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

    chunks = make("chunks", "chunk_id", "text", texts[:150], lambda n: {
        "speaker": ["S%d" % (i % 3) for i in range(n)], "start_ts_ms": [i * 10 for i in range(n)],
        "end_ts_ms": [i * 10 + 9 for i in range(n)]})
    arts = make("artifact_chunks", "artifact_chunk_id", "content", texts[150:], lambda n: {
        "artifact_id": [i // 3 for i in range(n)], "kind": ["summary"] * n})
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: False)
    gpu_be = None
    try:
        gpu_be = rt.GpuRetrieveBackend(chunks, arts, calls=calls, bm25_chunks=chunks.build_bm25_lane("text", positions=True),
                                       bm25_artifacts=arts.build_bm25_lane("content", positions=True))
        lanes = {"chunks": gpu_be._bm25["chunks"], "artifact_chunks": gpu_be._bm25["artifact_chunks"]}
        tables = {"chunks": chunks, "artifact_chunks": arts}
        oracles = {name: ClauseOracle([[lane.vocab[t] for t in tokenize(text)]
                                       for text in tables[name].columns[lane.text_column]]) for name, lane in lanes.items()}
        mode = {"syntax": False, "expand": False}

        def lane_rows(name, q, eligible, k):
            """(ids, score bits, count) of one query under the reading the settings select."""
            lane = lanes[name]
            if mode["syntax"]:
                try:
                    if mode["expand"]:
                        return predict(lane, oracles[name], lane.term_strings(), [q], k, eligible)
                    clauses, bag, _, _ = orc.read(q, expand=False)
                    eligible = oracles[name].passes([(kd, tuple(lane.vocab.get(t) for t in toks)) for kd, toks in clauses],
                                                    eligible)
                    q = " ".join(bag)
                except ValueError:                # over the limits: the bag reading of the raw string
                    pass
            return replay_index(lane, *lane.query_terms([q]), k, eligible)

        class CpuBackend(rt.RetrieveBackend):
            def resolve_call_ids(self, filters): return rt._resolve_call_ids(calls, filters)

            def _mask(self, table, f, c):
                m = table.filter_mask(f, c)
                return np.ones(len(table), bool) if m is None else m

            def _bm25(self, table, select, q, f, c, k):
                ids, bits, n = lane_rows(table.name, q, self._mask(table, f, c), k)
                pos = table._positions()
                return [{col: table.columns[col][pos[int(i)]] for col in select} | {"score": float(s)}
                        for i, s in zip(ids[0, :n[0]], bits[0, :n[0]].view(np.float32))]

            def fetch_chunks_bm25(self, q, f, c, k): return self._bm25(chunks, rt.CHUNK_SELECT, q, f, c, k)
            def fetch_artifacts_bm25(self, q, f, c, k): return self._bm25(arts, rt.ARTIFACT_SELECT, q, f, c, k)
            def estimate_dense_candidates(self, name, f, c): return int(self._mask(tables[name], f, c).sum())

        def response(req, be):
            resp = rt.retrieve_evidence(req, be)
            resp.pop("query_id")
            return resp
        nine = " ".join(f"{w}*" for w in ("de", "re", "co", "ti", "ga", "er", "st", "pr", "ro"))
        cases = [rt.RetrieveRequest(query="+deploy* -staging error", debug=True),
                 rt.RetrieveRequest(query="conection~ reset -time*", debug=True, return_style="ids_only"),
                 rt.RetrieveRequest(query='+gatewya~2 "the gateway" retry', debug=True,
                                    filters=rt.RetrieveFilters(call_ids=[calls[1]["call_id"], calls[4]["call_id"]])),
                 rt.RetrieveRequest(query="plain words about the connection", debug=True),
                 rt.RetrieveRequest(query=nine, debug=True)]
        got = {}
        for syntax, expand in ((False, False), (False, True), (True, False), (True, True)):
            monkeypatch.setattr(rt.settings, "bm25_query_syntax", syntax)
            monkeypatch.setattr(rt.settings, "bm25_query_expand", expand)
            mode["syntax"], mode["expand"] = syntax, syntax and expand
            for i, req in enumerate(cases):
                got[syntax, expand, i] = response(req, gpu_be)
                print(f"syntax={syntax} expand={expand} case {i}: {len(got[syntax, expand, i].get('quotes', []))} quotes")
                assert got[syntax, expand, i] == response(req, CpuBackend()), (syntax, expand, req)
        for i in range(len(cases)):
            assert got[False, True, i] == got[False, False, i]                   # the setting alone changes nothing
        assert got[True, True, 0] != got[True, False, 0] and got[True, True, 1] != got[True, False, 1]
        assert got[True, True, 3] == got[True, False, 3] == got[False, False, 3]  # no operator: the same response
        assert got[True, True, 4] == got[False, False, 4]                        # nine expanding items: the bag response
        hits = [q["chunk_id"] for q in got[True, True, 0]["quotes"]]
        assert hits and all("deploy" in texts[(i - 1000) // 2] and "staging" not in texts[(i - 1000) // 2] for i in hits)

        # HybridSearcher: the native lane reads the queries as the flags say
        lane = lanes["chunks"]
        qtexts = ["+deploy* error", "conection~ reset", "plain words error", "-the~ a~2 we~"]
        qv = torch.from_numpy(unit_rows(rng, 4)).to(DEV)
        want_on = predict(lane, oracles["chunks"], lane.term_strings(), qtexts, 20)
        want_off = replay_index(lane, *lane.query_terms(qtexts), 20)
        mode["syntax"], mode["expand"] = True, False
        want_syntax = [np.concatenate(x) for x in zip(*[lane_rows("chunks", q, None, 20) for q in qtexts])]
        for flags, want in ((dict(bm25_query_syntax=True, bm25_query_expand=True), want_on), (dict(), want_off),
                            (dict(bm25_query_expand=True), want_off), (dict(bm25_query_syntax=True), want_syntax)):
            out = HybridSearcher(chunks.index, None, dense_k=20, bm25_index=lane, bm25_k=20, **flags).search(qv, query_texts=qtexts)
            torch.cuda.synchronize()
            print(f"hybrid {flags}: bm25 counts {out['bm25_counts'].cpu().numpy().tolist()}")
            assert_equals_replay(want, out["bm25_ids"].cpu().numpy(), out["bm25_scores"].cpu().numpy(),
                                 out["bm25_counts"].cpu().numpy(), str(flags))
        assert not np.array_equal(want_on[0], want_off[0])
    finally:
        for lane in (getattr(gpu_be, "_bm25", {}) or {}).values():
            if hasattr(lane, "close"):
                lane.close()
        chunks.close(); arts.close()
