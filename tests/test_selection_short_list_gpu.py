"""The selection kernel on short candidate lists (crag_search.hip, finalize_fb_kernel: one block per query, a few dozen
candidates, k <= 24) and around the 64-candidate edge between its two searches for the k-th approximate score (ranking
by counting up to 64 candidates, the radix select beyond), against the plain fp32 scan (CRAG_NO_PREFILTER=1): ids,
score BITS and counts must be equal.  The selection adds its eight slice sums with DPP row shifts and reads the raw
query; the query preparation runs the fp64 butterfly of the query norm on the VALU and no longer stores fp32 fragments
for a prefilter search.  A change in the query norm moves both legs alike, so one case is pinned to ids and score bits
recorded from the commit before (tests/golden/selection_qnorm_k24.npz, scripts/probes/record_qnorm_golden.py).

[A short-list route of its own through the selection -- candidate g rescored by row group g, the k-th score and the
final ranking counted in registers -- was built with these tests behind a CRAG_FIN_NO_FAST switch as a third leg; it
measured slower and was taken out, and the leg went with it.]

32 768 rows is the smallest size that takes the prefilter on a 256-CU part.  Rows and queries have non-unit norms."""
import hashlib
import os
from pathlib import Path

import numpy as np
import pytest

from cadence_rag_amd.dense_index import DenseIndex
from tests.helpers import unit_rows

pytestmark = pytest.mark.gpu

ROWS, DIM, NQ_MAX = 32_768, 1024, 64
SWITCHES = ("CRAG_NO_PREFILTER", "CRAG_PF_WAITS", "CRAG_NO_RSPLIT", "CRAG_NO_FP16_MIRROR",
            "CRAG_PF_NT", "CRAG_PF_LAGS")
LEGS = {"default": {}, "plain": {"CRAG_NO_PREFILTER": "1"}}
GOLDEN = Path(__file__).parent / "golden" / "selection_qnorm_k24.npz"
GOLDEN_K = 24


def base_case():
    """the rows and the 64 queries every case starts from (the golden's inputs: the recording script calls this too):
    random directions, row norms in [0.1, 9], query norms spread over 1e-3 ... 1e3"""
    rng = np.random.default_rng(20_240)
    corpus = unit_rows(rng, ROWS) * rng.uniform(0.1, 9.0, (ROWS, 1)).astype(np.float32)
    norms = rng.permutation(np.logspace(-3.0, 3.0, NQ_MAX)).astype(np.float32)
    queries = unit_rows(rng, NQ_MAX) * norms[:, None]
    return np.ascontiguousarray(corpus), np.ascontiguousarray(queries)


def inputs_digest(corpus, queries):
    h = hashlib.sha256()
    h.update(corpus.tobytes())
    h.update(queries.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def _open(corpus, env):
    """a fresh index under `env` (the switches are read when it is created); the environment is left as it was"""
    saved = {key: os.environ.pop(key, None) for key in SWITCHES}
    os.environ.update(env)
    try:
        ix = DenseIndex(corpus.shape[1], capacity=len(corpus))
        ix.add(corpus)
        return ix
    finally:
        for key in SWITCHES:
            os.environ.pop(key, None)
            if saved[key] is not None:
                os.environ[key] = saved[key]


def _legs(corpus):
    out = {}
    try:
        for leg, env in LEGS.items():
            out[leg] = _open(corpus, env)
    except Exception:
        for ix in out.values():
            ix.close()
        raise
    return out


def _close(ixs):
    for ix in ixs.values():
        ix.close()


def _same(x, y):
    """ids, score BITS and counts"""
    return (np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32))
            and np.array_equal(x[2], y[2]))


def _compare(ixs, q, k, packed, what):
    """one search per leg: bit-equal; returns the default leg's answer and its statistics"""
    res, stats = {}, {}
    for leg, ix in ixs.items():
        ix.prefilter_stats()   # (reading resets)
        res[leg] = ix.search(q, k, row_mask=packed)
        stats[leg] = ix.prefilter_stats()
        if leg == "plain":
            assert "prefilter" not in ix.last_scan_kernel(), (what, ix.last_scan_kernel())
        else:
            assert ix.last_scan_kernel().startswith("crag::prefilter_kernel<"), (what, ix.last_scan_kernel())
    print(f"\n{what}: {stats['default']}")
    assert _same(res["default"], res["plain"]), what
    return res["default"], stats["default"]


def _check_tail(ids, scores, counts, k):
    for i, c in enumerate(counts):
        assert np.all(ids[i, :c] >= 0) and not np.isnan(scores[i, :c]).any()
        assert np.all(ids[i, c:] == -1) and np.all(scores[i, c:].view(np.uint32) == 0x7FC00000)
    assert ids.shape[1] == k


@pytest.fixture(scope="module")
def base(gpu):
    return base_case()


@pytest.fixture(scope="module")
def legs(base):
    corpus, queries = base
    ixs = _legs(corpus)
    yield corpus, queries, ixs
    _close(ixs)


# ---- case 1: across the 64-candidate edge ---------------------------------------------------------------------------
PLANTED = (0, 5, 10, 11, 40, 56, 64, 65, 72, 90)


@pytest.fixture(scope="module")
def edge(base):
    """m rows at cosine 0.9 +- 1e-4 to one query over the random background (whose cosines stay below 0.2), for every
    m: all m lie within 2 delta = 2.5e-3 of each other, hence of the k-th for m >= k.  One search per leg and m.
    Where they are planted: in tiles drawn at random, at row positions whose residues mod 32 run through permutations
    of 0 .. 31.  The scan's bound is the k-th largest of the 32 class maxima (class = row position mod 32,
    crag_search.hip): planted rows that share a class lift one maximum only, and with fewer than k classes lifted the
    bound stays at the background's level and lets a hundred background rows through at this size (four tiles per
    workgroup), whatever m is -- the list would never be short."""
    corpus, _ = base
    k = 10
    rng = np.random.default_rng(64)
    u = unit_rows(rng, 1)[0]
    w = unit_rows(rng, max(PLANTED))
    w -= np.outer(w @ u, u)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    c = (0.9 + 1e-4 * rng.uniform(-1.0, 1.0, max(PLANTED))).astype(np.float32)
    rows = (c[:, None] * u[None] + np.sqrt(1.0 - c * c)[:, None] * w).astype(np.float32)
    rows *= rng.uniform(0.1, 9.0, (len(rows), 1)).astype(np.float32)
    tiles = rng.choice(ROWS // 32, max(PLANTED), replace=False)
    where = tiles * 32 + np.concatenate([rng.permutation(32) for _ in range(3)])[:max(PLANTED)]
    q = (u * np.float32(3.7))[None]
    out = {}
    for m in PLANTED:
        planted = corpus.copy()
        planted[where[:m]] = rows[:m]
        ixs = _legs(planted)
        try:
            res, stats = _compare(ixs, q, k, None, f"planted m={m}")
        finally:
            _close(ixs)
        out[m] = (res, stats, set(where[:m].tolist()))
    return k, out


@pytest.mark.parametrize("m", PLANTED)
def test_selection_agrees_with_the_plain_scan_across_the_64_candidate_edge(edge, m):
    k, out = edge
    (ids, scores, counts), stats, planted = out[m]
    assert counts[0] == k
    assert set(ids[0, :min(m, k)].tolist()) <= planted           # (ids are row positions here)
    if m >= k:   # every planted row lies within 2 delta of the k-th and no background row does
        assert stats["rescored_rows"] == m, stats
    assert stats["searches"] == 1, stats


def test_the_edge_is_crossed(edge):
    """m = 90 must have had more than 64 candidates (the radix select), one of m <= 10 at most 64 (ranking by counting)"""
    _, out = edge
    cands = {m: out[m][1]["candidates"] for m in PLANTED}
    assert cands[90] > 64, cands
    if not any(cands[m] <= 64 for m in PLANTED if m <= 10):
        pytest.fail(f"no case of m <= 10 had a short candidate list: {cands}")


# ---- case 2: ties ---------------------------------------------------------------------------------------------------
def test_ties_come_out_in_id_order(base):
    corpus, queries = base
    rng = np.random.default_rng(30)
    tied = corpus.copy()
    where = np.sort(rng.choice(ROWS, 30, replace=False))
    tied[where] = queries[7] * np.float32(0.25)     # 30 identical rows, cosine 1 to query 7
    ixs = _legs(tied)
    try:
        (ids, scores, counts), _ = _compare(ixs, queries[7:8], 10, None, "30 tied rows")
    finally:
        _close(ixs)
    assert counts[0] == 10
    assert ids[0].tolist() == where[:10].tolist()
    assert np.all(scores[0].view(np.uint32) == scores[0, :1].view(np.uint32))


# ---- case 3: short lists --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 33, 64])
def test_short_lists_and_empty_answers(legs, nq):
    corpus, queries, ixs = legs
    k = 10
    q = queries[:nq].copy()
    if nq > 1:
        q[1] = 0.0   # a zero query among real ones
    real = [i for i in range(nq) if not (nq > 1 and i == 1)]
    three = np.zeros(ROWS, dtype=bool)
    three[[17, 9_999, ROWS - 1]] = True
    (ids, scores, counts), _ = _compare(ixs, q, k, DenseIndex.pack_mask(three), f"nq={nq} three eligible rows")
    _check_tail(ids, scores, counts, k)
    assert np.all(counts[real] == 3)
    for i in real:
        assert sorted(ids[i, :3].tolist()) == [17, 9_999, ROWS - 1]
    (ids, scores, counts), _ = _compare(ixs, q, k, DenseIndex.pack_mask(np.zeros(ROWS, dtype=bool)), f"nq={nq} no eligible row")
    _check_tail(ids, scores, counts, k)
    assert np.all(counts == 0)
    (ids, scores, counts), _ = _compare(ixs, q, k, None, f"nq={nq} zero query")
    _check_tail(ids, scores, counts, k)
    assert np.all(counts[real] == k)
    if nq > 1:
        assert counts[1] == 0
    else:
        (ids, scores, counts), _ = _compare(ixs, np.zeros((1, DIM), dtype=np.float32), k, None, "a lone zero query")
        _check_tail(ids, scores, counts, k)
        assert counts[0] == 0


# ---- case 4: sweep of k and nq --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 24, 25])
@pytest.mark.parametrize("nq", [1, 33, 64])
def test_sweep_of_k_and_nq(legs, nq, k):
    """k <= 24: one class set; k = 25: two"""
    corpus, queries, ixs = legs
    (ids, _, counts), _ = _compare(ixs, queries[:nq], k, None, f"nq={nq} k={k}")
    assert np.all(counts == k) and np.all(ids >= 0)


# ---- case 5: state hand-over ----------------------------------------------------------------------------------------
def test_the_workspace_is_left_clean(legs):
    """the same search twice, then k = 10 / 50 / 10 on the same index: every answer is the fp32 scan's"""
    corpus, queries, ixs = legs
    first = None
    for step, k in enumerate((10, 10, 10, 50, 10)):
        got = ixs["default"].search(queries, k)
        assert _same(got, ixs["plain"].search(queries, k)), (step, k)
        if k == 10:
            first = first or got
            assert _same(got, first), step


# ---- case 6: the bits of the query norm -----------------------------------------------------------------------------
def test_results_equal_the_recording_of_the_commit_before(legs):
    corpus, queries, ixs = legs
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["inputs_sha256"], inputs_digest(corpus, queries)), \
        "the generated inputs are not the recorded ones (a changed random generator, not a changed kernel)"
    for leg, ix in ixs.items():
        ids, scores, counts = ix.search(queries, GOLDEN_K)
        assert np.array_equal(ids, gold["ids"]), leg
        assert np.array_equal(scores.view(np.uint32), gold["score_bits"]), leg
        assert np.all(counts == GOLDEN_K), leg
