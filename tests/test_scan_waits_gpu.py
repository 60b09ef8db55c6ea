"""The two wait schedules of the fp16-mirror prefilter scan (crag_search.hip, prefilter_kernel's FRAG parameter):
CRAG_PF_WAITS=tile waits for a whole tile in front of its MFMAs, =fragment waits for each k-step's own fragment and
re-issues its register at once.  Only the moment a load is waited for differs, so ids, scores and counts must be
bit-equal between the two and equal to the plain fp32 scan (CRAG_NO_PREFILTER=1), and the rows rescored exactly --
a function of the scores alone (the rescored-rows invariant) -- must be the same number.  Candidate
counts depend on timing and are not compared.

Row counts, for 256 workgroups: 32 768 = the smallest prefilter size, four tiles per workgroup (every tile is a
stashed tile, the loop ends on the early bound read); 41 000 = five to six tiles, ragged last tile; 100 000 = twelve
and thirteen tiles mixed.  nq 1 / 32 take the 32-query kernels, 33 / 64 the 64-query ones; k 1, 10, 24 one class set,
25 two, 100 four.  Every case runs without a mask, with a shared mask and with per-query masks (extra loads in front
of the waits)."""
import os

import numpy as np
import pytest

from cadence_rag_amd.dense_index import DenseIndex
from tests.helpers import unit_rows

pytestmark = pytest.mark.gpu

SWITCHES = ("CRAG_PF_WAITS", "CRAG_NO_PREFILTER", "CRAG_NO_RSPLIT", "CRAG_NO_FP16_MIRROR", "CRAG_PF_NT", "CRAG_PF_LAGS")
LEGS = {"tile": {"CRAG_PF_WAITS": "tile"}, "fragment": {"CRAG_PF_WAITS": "fragment"}, "plain": {"CRAG_NO_PREFILTER": "1"}}
NQ_MAX = 64


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


def _three(corpus):
    out = {}
    try:
        for leg, env in LEGS.items():
            out[leg] = _open(corpus, env)
    except Exception:
        for ix in out.values():
            ix.close()
        raise
    return out


@pytest.fixture(scope="module", params=[32_768, 41_000, 100_000])
def legs(request, gpu):
    """per row count, built once: the corpus, the queries, a shared and a per-query mask, and the three indices"""
    n = request.param
    rng = np.random.default_rng(n)
    corpus = unit_rows(rng, n) * rng.uniform(0.1, 9.0, (n, 1)).astype(np.float32)
    q = rng.standard_normal((NQ_MAX, 1024)).astype(np.float32)
    shared = DenseIndex.pack_mask(rng.random(n) < 0.3)
    per_query = rng.random((NQ_MAX, n)) < 0.5
    ixs = _three(corpus)
    yield n, q, shared, per_query, ixs
    for ix in ixs.values():
        ix.close()


def _compare(ixs, q, k, packed, what):
    """one search per leg: results bit-equal over all three, rescored rows equal between the two schedules"""
    res, stats = {}, {}
    for leg, ix in ixs.items():
        ix.prefilter_stats()   # (reading resets)
        res[leg] = ix.search(q, k, row_mask=packed)
        stats[leg] = ix.prefilter_stats()
        if leg == "plain":
            assert "prefilter" not in ix.last_scan_kernel(), (what, ix.last_scan_kernel())
            assert ix.scan_waits() == "tile"
        else:
            # the name is the four-argument one whatever the schedule; the schedule has a getter of its own
            assert ix.last_scan_kernel().startswith("crag::prefilter_kernel<"), (what, ix.last_scan_kernel())
            assert ix.last_scan_kernel().endswith("true, false>"), (what, ix.last_scan_kernel())
            assert ix.scan_waits() == leg, (what, ix.scan_waits())
    for other in ("fragment", "plain"):
        for x, y in zip(res["tile"], res[other]):
            assert np.array_equal(x, y, equal_nan=True), (what, other)
    print(f"\n{what}: tile {stats['tile']}, fragment {stats['fragment']}")
    # (a search the overflow fallback answered counts nothing: at 32 768 rows the two-set bound of k = 25 rests on one
    # tile per workgroup and lets too many rows pass, under either schedule)
    assert stats["tile"]["searches"] == stats["fragment"]["searches"], (what, stats)
    assert stats["tile"]["rescored_rows"] == stats["fragment"]["rescored_rows"], (what, stats)
    return res["fragment"]


@pytest.mark.parametrize("k", [1, 10, 24, 25, 100])
@pytest.mark.parametrize("nq", [1, 32, 33, 64])
def test_both_wait_schedules_and_the_plain_scan_agree(legs, nq, k):
    n, q, shared, per_query, ixs = legs
    for name, packed in (("no mask", None), ("shared mask", shared),
                         ("per-query masks", DenseIndex.pack_mask(per_query[:nq]))):
        ids, _, counts = _compare(ixs, q[:nq], k, packed, f"rows={n} nq={nq} k={k} {name}")
        assert np.all(counts == k) and np.all(ids >= 0)


def test_zero_and_nan_rows_stay_out_under_both_schedules(gpu):
    rng = np.random.default_rng(77)
    n = 41_000
    corpus = unit_rows(rng, n)
    zero, bad = [0, 31, 32, 20_000, n - 1], [5, 8_191, 8_192, 33_333, n - 2]
    corpus[zero] = 0.0
    for i, r in enumerate(bad):
        corpus[r, (7 * i) % 1024] = np.nan
    q = rng.standard_normal((NQ_MAX, 1024)).astype(np.float32)
    q[3] = 0.0   # a query that matches nothing
    mask = rng.random((NQ_MAX, n)) < 0.5
    ixs = _three(corpus)
    try:
        for nq, k in ((64, 10), (33, 25), (7, 100)):
            for packed in (None, DenseIndex.pack_mask(mask[:nq])):
                ids, _, _ = _compare(ixs, q[:nq], k, packed, f"zero/NaN rows nq={nq} k={k} mask={packed is not None}")
                assert not np.isin(ids, zero + bad).any()
    finally:
        for ix in ixs.values():
            ix.close()


def test_overflowing_search_still_answered_by_the_fallback_under_both_schedules(gpu):
    """20 000 identical rows: the candidate list of the query next to them overflows and the fallback blocks of the
    selection launch answer (no search counted), whichever schedule the scan ran with."""
    rng = np.random.default_rng(5)
    n = 60_000
    corpus = unit_rows(rng, n)
    corpus[20_000:40_000] = corpus[7]
    others = rng.standard_normal((39, 1024)).astype(np.float32)
    others -= np.outer(others @ corpus[7], corpus[7])
    q = np.concatenate([corpus[7][None] * 2.0, others])
    ixs = _three(corpus)
    try:
        ids, scores, _ = _compare(ixs, q, 10, None, "overflow")
        assert ids[0].tolist() == [7] + list(range(20_000, 20_009))
        assert np.all(scores[0] == scores[0, 0])
        for leg in ("tile", "fragment"):
            ixs[leg].prefilter_stats()
            assert np.array_equal(ixs[leg].search(q[1:], 10)[0], ids[1:])   # the next search starts clean
            assert ixs[leg].prefilter_stats()["searches"] == 1
    finally:
        for ix in ixs.values():
            ix.close()
