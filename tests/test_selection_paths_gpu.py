"""Every path through the selection launch (crag_search.hip, finalize_fb_kernel), each against the plain fp32 scan
(an index created under CRAG_NO_PREFILTER=1): ids, score BITS and counts must be equal.  The kernel's text is laid out
for the common search -- k <= 24, one block per query, at most 64 candidates -- and everything else sits behind that
run of code: the radix select (more than 64 candidates), the hand-off and gather of several blocks per query (k > 32),
the fallback role (a candidate list that overflows) and the short answers (fewer eligible rows than k).  Each case
asserts through prefilter_stats() that the path it means was the one taken.

The corpus is the smallest that takes the prefilter: one workgroup per CU, PF_MIN_ROWS_PER_GROUP = 128 rows each.  At
that size a scan workgroup has four tiles, all of them scored before a bound from the other workgroups can arrive, so a
few hundred background rows pass per query whatever the data looks like (measured: 257 candidates for one query at
k = 24 with 32 planted rows far above the background), and a k > 32 search, whose bound is weaker still, overflows its
list.  The cases that need a list of a given length therefore bound it with a row mask, which the scan applies and
the selection never sees: a query's candidates are eligible rows, so

  * 48 eligible rows: at most 48 candidates for every query -- the common path.  `candidates` is a sum over the
    queries, but the bound holds per query because it comes from the mask, not from the sum; every query has at least
    k (its exact top-k are candidates).  The 48 rows are taken from 200 planted at cosine 0.9 +- 1e-4 to query 0: all
    within 2 delta = 2.5e-3 of one another, so query 0 has all 48 -- more than k: its k-th score is searched for.
    (delta is the proven worst case of the fp16 scores' error; on rows like these the error is a few 1e-5, so the
    2e-4 the cosines spread over and the error together stay ten times inside the window.  The same reading as
    test_selection_short_list_gpu.py's planted rows.)
  * the 200 planted rows unmasked, k = 10: all 200 are candidates of query 0 -- the radix select.
  * 2 000 eligible rows, k = 33 / 100: no overflow, four or eight blocks per query.
"""
import os

import numpy as np
import pytest

from cadence_rag_amd.dense_index import DenseIndex
from tests.helpers import unit_rows

pytestmark = pytest.mark.gpu

DIM, NQ = 1024, 64
PF_MIN_ROWS_PER_GROUP = 128     # crag_kernels.h
CAP = 8192                      # candidates per query (plan_search, k <= 104)
SWITCHES = ("CRAG_NO_PREFILTER", "CRAG_PF_WAITS", "CRAG_NO_RSPLIT", "CRAG_NO_FP16_MIRROR", "CRAG_PF_NT", "CRAG_PF_LAGS")


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


class Legs:
    """the same rows behind the prefilter path and behind the plain fp32 scan"""

    def __init__(self, corpus):
        self.default = _open(corpus, {})
        try:
            self.plain = _open(corpus, {"CRAG_NO_PREFILTER": "1"})
        except Exception:
            self.default.close()
            raise

    def close(self):
        self.default.close()
        self.plain.close()

    def compare(self, q, k, what, packed=None):
        """one search per leg, bit-equal; returns the prefilter leg's answer and its statistics"""
        want = self.plain.search(q, k, row_mask=packed)
        assert "prefilter" not in self.plain.last_scan_kernel(), (what, self.plain.last_scan_kernel())
        self.default.prefilter_stats()   # (reading resets)
        got = self.default.search(q, k, row_mask=packed)
        stats = self.default.prefilter_stats()
        assert self.default.last_scan_kernel().startswith("crag::prefilter_kernel<"), (what, self.default.last_scan_kernel())
        print(f"\n{what}: {stats}")
        assert np.array_equal(got[0], want[0]), what
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what
        assert np.array_equal(got[2], want[2]), what
        return got, stats


def _toward(rng, u, cos):
    """rows at the given cosines to the unit vector u, with norms in [0.1, 9]"""
    w = unit_rows(rng, len(cos))
    w -= np.outer(w @ u, u)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    c = np.asarray(cos, dtype=np.float64)
    rows = c[:, None] * u[None].astype(np.float64) + np.sqrt(1.0 - c * c)[:, None] * w
    return (rows * rng.uniform(0.1, 9.0, (len(cos), 1))).astype(np.float32)


def _spread(rng, rows, n):
    """n row positions in tiles drawn at random whose residues mod 32 run through permutations of 0 .. 31"""
    tiles = rng.choice(rows // 32, n, replace=False)
    return tiles * 32 + np.concatenate([rng.permutation(32) for _ in range((n + 31) // 32)])[:n]


@pytest.fixture(scope="module")
def size(gpu):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * PF_MIN_ROWS_PER_GROUP


@pytest.fixture(scope="module")
def background(size):
    rng = np.random.default_rng(2_610)
    corpus = unit_rows(rng, size) * rng.uniform(0.1, 9.0, (size, 1)).astype(np.float32)
    units = unit_rows(rng, NQ)
    norms = rng.permutation(np.logspace(-2.0, 2.0, NQ)).astype(np.float32)
    return np.ascontiguousarray(corpus), units, np.ascontiguousarray(units * norms[:, None])


# ---- more than 64 candidates: the radix select, one round -------------------------------------------------------------
@pytest.fixture(scope="module")
def cluster(background, size):
    """200 rows at cosine 0.9 +- 1e-4 to query 0: all within 2 delta of the 10th best, so all of them are candidates"""
    corpus, units, queries = background
    rng = np.random.default_rng(2_612)
    planted = corpus.copy()
    where = _spread(rng, size, 200)
    planted[where] = _toward(rng, units[0], 0.9 + 1e-4 * rng.uniform(-1.0, 1.0, 200))
    legs = Legs(planted)
    yield queries, legs, set(where.tolist())
    legs.close()


@pytest.mark.parametrize("nq", [1, 64])
def test_radix_select(cluster, nq):
    queries, legs, where = cluster
    k = 10
    (ids, _, counts), stats = legs.compare(queries[:nq], k, f"cluster nq={nq}")
    assert np.all(counts == k)
    assert set(ids[0].tolist()) <= where
    assert stats["searches"] == 1, stats
    assert stats["rescored_rows"] >= 200, stats
    if nq == 1:
        assert 64 < stats["candidates"] <= 4096, stats   # the radix select, all candidates in one round


# ---- the common path: at most 64 candidates, one block per query ------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 24])
@pytest.mark.parametrize("nq", [1, 33, 64])
def test_common_path(cluster, size, nq, k):
    queries, legs, where = cluster
    some = np.zeros(size, dtype=bool)
    some[sorted(where)[::4][:48]] = True
    (ids, _, counts), stats = legs.compare(queries[:nq], k, f"common nq={nq} k={k}", DenseIndex.pack_mask(some))
    assert np.all(counts == k) and np.all(some[ids])
    assert stats["searches"] == 1, stats
    assert nq * k <= stats["candidates"] <= nq * 48, stats
    if nq == 1:
        assert stats["candidates"] == 48, stats


# ---- k > 32: several blocks per query, hand-off and gather ------------------------------------------------------------
@pytest.mark.parametrize("k", [33, 100])
@pytest.mark.parametrize("nq", [1, 64])
def test_several_blocks_per_query(cluster, size, nq, k):
    """plan_search: rsplit = 8 up to 16 queries, 4 up to 128"""
    queries, legs, _ = cluster
    some = np.zeros(size, dtype=bool)
    some[np.random.default_rng(2_614).choice(size, 2_000, replace=False)] = True
    (ids, _, counts), stats = legs.compare(queries[:nq], k, f"split nq={nq} k={k}", DenseIndex.pack_mask(some))
    assert np.all(counts == k) and np.all(some[ids])
    assert stats["searches"] == 1, stats      # (an overflow would have left it at 0)
    assert nq * k <= stats["rescored_rows"] <= stats["candidates"] <= nq * 2_000, stats


# ---- overflow: the fallback role --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 33])
def test_fallback_role(background, size, nq):
    corpus, units, queries = background
    rng = np.random.default_rng(2_613)
    same = corpus.copy()
    where = np.sort(rng.choice(size, 20_000, replace=False))
    same[where] = units[0] * np.float32(0.25)   # 20 000 identical rows, cosine 1 to query 0: more than the list holds
    legs = Legs(same)
    try:
        (ids, scores, counts), stats = legs.compare(queries[:nq], 10, f"overflow nq={nq}")
        assert stats["searches"] == 0, stats    # no selection block answered: the fallback blocks did
        assert counts[0] == 10 and ids[0].tolist() == where[:10].tolist()
        assert np.all(scores[0].view(np.uint32) == scores[0, :1].view(np.uint32))
        # the workspace is left clean: a search that does not overflow, on the same index
        _, stats = legs.compare(queries[1:2], 10, "after the overflow")
        assert stats["searches"] == 1, stats
    finally:
        legs.close()


# ---- fewer eligible rows than k ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 64])
def test_fewer_eligible_rows_than_k(cluster, size, nq):
    queries, legs, _ = cluster
    k = 10
    three = np.zeros(size, dtype=bool)
    three[[17, size // 3, size - 1]] = True
    (ids, scores, counts), stats = legs.compare(queries[:nq], k, f"three eligible rows nq={nq}", DenseIndex.pack_mask(three))
    assert stats["searches"] == 1 and stats["candidates"] <= 3 * nq, stats
    assert np.all(counts == 3)
    for i in range(nq):
        assert sorted(ids[i, :3].tolist()) == [17, size // 3, size - 1]
        assert not np.isnan(scores[i, :3]).any()
        assert np.all(ids[i, 3:] == -1) and np.all(scores[i, 3:].view(np.uint32) == 0x7FC00000)
