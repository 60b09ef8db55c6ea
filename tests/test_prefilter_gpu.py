"""The fp16-prefilter + exact-rescoring search path (crag_search.hip: prefilter_kernel / finalize_kernel) against
the plain fp32 scan of the same library (CRAG_NO_PREFILTER=1) — bit for bit — and against the CPU oracle, on
inputs built to stress the proven error bound, the candidate lists and the overflow fallback."""
import numpy as np
import pytest

import oracle
from cadence_rag_amd.dense_index import DenseIndex
from tests.helpers import assert_topk_matches, unit_rows

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _index(corpus, monkeypatch, prefilter=True, ids=None):
    if prefilter:
        monkeypatch.delenv("CRAG_NO_PREFILTER", raising=False)
    else:
        monkeypatch.setenv("CRAG_NO_PREFILTER", "1")   # read once, when the index is created
    ix = DenseIndex(corpus.shape[1], capacity=len(corpus))
    ix.add(corpus, ids=ids)
    return ix


def test_fp16_mirror_scan_equals_the_scan_of_the_fp32_rows(gpu, monkeypatch):
    """The mirror holds exactly the operand the scan of the fp32 rows builds in registers (same multiply, same
    rounding), so both prefilter scans feed the exact rescoring the same way: identical results, also after rows
    were overwritten in place, and a row that may never match (zero norm) stays out through its NaN mirror."""
    rng = np.random.default_rng(91)
    n = 44_000
    corpus = unit_rows(rng, n) * rng.uniform(0.1, 9.0, (n, 1)).astype(np.float32)
    corpus[123] = 0.0
    q = rng.standard_normal((64, 1024)).astype(np.float32)
    fresh = unit_rows(rng, 500)
    out = {}
    for mirror in (True, False):
        if mirror:
            monkeypatch.delenv("CRAG_NO_FP16_MIRROR", raising=False)
        else:
            monkeypatch.setenv("CRAG_NO_FP16_MIRROR", "1")
        ix = _index(corpus, monkeypatch)
        try:
            assert ix.prefilter_row_bytes() == (2048 if mirror else 4096)
            first = ix.search(q, 10)
            assert ("true" in ix.last_scan_kernel()) == mirror, ix.last_scan_kernel()
            ix.update(20_000, fresh)
            out[mirror] = (first, ix.search(q, 10), ix.search(q[:7], 100))
        finally:
            ix.close()
    for a, b in zip(out[True], out[False]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    assert 123 not in out[True][0][0]
    after = corpus.copy()
    after[20_000:20_500] = fresh
    want = oracle.exact_topk(q[:3], after, 10, mode=oracle.F64, fast=True)
    assert_topk_matches(out[True][1][0][:3], out[True][1][1][:3], out[True][1][2][:3], *want, tol=TOL)


@pytest.mark.parametrize("nq,k", [(64, 10), (20, 40), (64, 100)])
def test_streaming_cache_policy_changes_nothing_but_the_loads(gpu, monkeypatch, nq, k):
    """Mirrors above 1.5 GB are scanned with non-temporal loads (another template instance of the kernel); forced
    here on a small corpus: same results, and the kernel name says which instance ran."""
    rng = np.random.default_rng(300 + nq + k)
    corpus = unit_rows(rng, 40_000)
    q = rng.standard_normal((nq, 1024)).astype(np.float32)
    out = {}
    for nt in ("0", "1"):
        monkeypatch.setenv("CRAG_PF_NT", nt)
        ix = _index(corpus, monkeypatch)
        try:
            out[nt] = ix.search(q, k)
            assert ix.last_scan_kernel().endswith("true, true>" if nt == "1" else "true, false>"), ix.last_scan_kernel()
        finally:
            ix.close()
    monkeypatch.delenv("CRAG_PF_NT")
    for a, b in zip(out["0"], out["1"]):
        assert np.array_equal(a, b, equal_nan=True)
    want = oracle.exact_topk(q[:3], corpus, k, mode=oracle.F64, fast=True)
    assert_topk_matches(out["1"][0][:3], out["1"][1][:3], out["1"][2][:3], *want, tol=TOL)


def _both(corpus, q, k, monkeypatch, mask=None):
    packed = None if mask is None else DenseIndex.pack_mask(mask)
    out = []
    for pf in (True, False):
        ix = _index(corpus, monkeypatch, prefilter=pf)
        try:
            res = [ix.search(q, k, row_mask=packed) for _ in range(2)]   # forward and reversed pass
            assert "prefilter" in ix.last_scan_kernel() if pf else "prefilter" not in ix.last_scan_kernel()
            for a, b in zip(res[0], res[1]):
                assert np.array_equal(a, b, equal_nan=True)
            out.append(res[0])
        finally:
            ix.close()
    return out


@pytest.mark.parametrize("n,nq,k", [(40_000, 64, 10), (40_000, 1, 10), (50_001, 32, 10), (45_000, 33, 50),
                                    (60_000, 64, 100), (33_000, 7, 128), (70_000, 100, 24), (36_000, 64, 25)])
def test_prefilter_path_equals_fp32_scan_bit_for_bit(gpu, monkeypatch, n, nq, k):
    rng = np.random.default_rng(n + nq * 7 + k)
    corpus = unit_rows(rng, n) * rng.uniform(0.05, 20.0, (n, 1)).astype(np.float32)   # raw rows, any scale
    q = rng.standard_normal((nq, 1024)).astype(np.float32) * 3.0
    new, old = _both(corpus, q, k, monkeypatch)
    assert np.array_equal(new[0], old[0])                       # same ids, same order
    assert np.array_equal(new[1], old[1], equal_nan=True)       # the rescoring redoes the scan's fp32 chain exactly
    assert np.array_equal(new[2], old[2])
    want = oracle.exact_topk(q[:4], corpus, k, mode=oracle.F64, fast=True)
    assert_topk_matches(new[0][:4], new[1][:4], new[2][:4], *want, tol=TOL)


@pytest.mark.parametrize("frac,per_query,nq,k", [(0.5, True, 64, 10), (0.02, True, 40, 50), (0.3, False, 32, 10),
                                                 (0.0005, True, 64, 10)])
def test_prefilter_path_with_row_masks(gpu, monkeypatch, frac, per_query, nq, k):
    rng = np.random.default_rng(int(frac * 1e4) + nq)
    n = 48_000
    corpus = unit_rows(rng, n)
    q = rng.standard_normal((nq, 1024)).astype(np.float32)
    mask = rng.random((nq, n) if per_query else (n,)) < frac
    new, old = _both(corpus, q, k, monkeypatch, mask=mask)
    for a, b in zip(new, old):
        assert np.array_equal(a, b, equal_nan=True)
    m8 = np.packbits(mask[:3] if per_query else mask, axis=-1, bitorder="little")
    want = oracle.exact_topk(q[:3], corpus, k, mask=m8, mode=oracle.F64, fast=True)
    assert_topk_matches(new[0][:3], new[1][:3], new[2][:3], *want, tol=TOL)


def test_contiguous_scope_mask_like_a_date_range(gpu, monkeypatch):
    """A date filter on a time-ordered table selects a contiguous row range that a single workgroup may own:
    the bounds must still form (they are kept per row class, not per workgroup)."""
    rng = np.random.default_rng(8)
    n = 80_000
    corpus = unit_rows(rng, n)
    q = rng.standard_normal((64, 1024)).astype(np.float32)
    mask = np.zeros(n, dtype=bool)
    mask[41_000:41_300] = True          # 300 rows: inside one workgroup's range
    mask[70_000:70_020] = True
    new, old = _both(corpus, q, 10, monkeypatch, mask=mask)
    for a, b in zip(new, old):
        assert np.array_equal(a, b, equal_nan=True)
    assert set(new[0].ravel().tolist()) <= set(range(41_000, 41_300)) | set(range(70_000, 70_020))


def test_dense_near_ties_stress_the_error_bound(gpu, monkeypatch):
    """Thousands of rows whose true cosines to the queries lie within a few 1e-4 of each other around the k-th
    best: a prefilter whose error bound were too optimistic would drop true neighbours here.  Rows are built to
    bias fp16 rounding (components just below rounding boundaries)."""
    rng = np.random.default_rng(77)
    n, d = 40_000, 1024
    base = rng.standard_normal(d).astype(np.float32)
    base /= np.linalg.norm(base)
    corpus = unit_rows(rng, n)
    cluster = base[None, :] + 2e-3 * rng.standard_normal((6000, d)).astype(np.float32)
    # push every component towards the upper end of its fp16 rounding interval (worst-case one-sided error)
    h = cluster.astype(np.float16).astype(np.float32)
    ulp = np.abs(np.spacing(cluster.astype(np.float16)).astype(np.float32))
    cluster = (h + 0.499 * ulp * np.sign(h)).astype(np.float32)
    corpus[10_000:16_000] = cluster
    q = np.stack([base, base + 1e-3 * rng.standard_normal(d).astype(np.float32), -base] +
                 [rng.standard_normal(d).astype(np.float32) for _ in range(29)])
    for k in (10, 100):
        new, old = _both(corpus, q, k, monkeypatch)
        for a, b in zip(new, old):
            assert np.array_equal(a, b, equal_nan=True)
        want = oracle.exact_topk(q[:3], corpus, k, mode=oracle.F64, fast=True)
        assert_topk_matches(new[0][:3], new[1][:3], new[2][:3], *want, tol=TOL)


def test_candidate_overflow_falls_back_to_the_exact_scan(gpu, monkeypatch):
    """20 000 identical rows (boilerplate chunks embed identically): every one of them is within the bound of
    the k-th best, the candidate list (8192 per query) overflows, the gated fp32 scan takes over: the answer
    is the first k duplicates by id, as the oracle says."""
    rng = np.random.default_rng(5)
    n = 60_000
    corpus = unit_rows(rng, n)
    corpus[20_000:40_000] = corpus[7]
    others = rng.standard_normal((39, 1024)).astype(np.float32)
    others -= np.outer(others @ corpus[7], corpus[7])   # orthogonal to the duplicated row: it never nears their top-k
    q = np.concatenate([corpus[7][None] * 2.0, others])
    ix = _index(corpus, monkeypatch)
    try:
        ids, scores, counts = ix.search(q, 10)
        assert "prefilter" in ix.last_scan_kernel()
        assert ids[0].tolist() == [7] + list(range(20_000, 20_009))
        assert np.all(scores[0] == scores[0, 0])
        stats = ix.prefilter_stats()
        assert stats["searches"] == 0           # the finalize kernel merged the fp32 scan's lists instead
        want = oracle.exact_topk(q[:4], corpus, 10, mode=oracle.F64, fast=True)
        assert_topk_matches(ids[:4], scores[:4], counts[:4], *want, tol=TOL)
        # the next search on the same workspace starts clean
        ids2, _, _ = ix.search(q[1:], 10)
        assert np.array_equal(ids2, ids[1:])
        assert ix.prefilter_stats()["searches"] == 1
    finally:
        ix.close()


def test_candidate_statistics_stay_near_k(gpu, monkeypatch):
    """Byte accounting behind bench.py's roofline: on the bench's corpus shape the filter passes a few dozen rows
    per query and rescoring touches about k + a few of them."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    c = torch.randn(100_000, 1024, generator=g, device=dev)
    c /= c.norm(dim=1, keepdim=True)
    q = torch.randn(64, 1024, generator=g, device=dev)
    monkeypatch.delenv("CRAG_NO_PREFILTER", raising=False)
    with DenseIndex(1024, capacity=100_000) as ix:
        ix.add(c)
        for k, cand_max, resc_max in ((10, 400, 40), (50, 1200, 120), (100, 2500, 220)):
            ix.prefilter_stats()
            for _ in range(4):
                ix.search(q, k)
            s = ix.prefilter_stats()
            per_query_c = s["candidates"] / s["searches"] / 64
            per_query_r = s["rescored_rows"] / s["searches"] / 64
            print(f"\nk={k}: candidates/query {per_query_c:.1f}, rescored rows/query {per_query_r:.1f}")
            assert s["searches"] == 4 and k <= per_query_r <= resc_max and per_query_c <= cand_max


def test_rows_with_extreme_norms_keep_the_index_on_the_fp32_scan(gpu, monkeypatch):
    rng = np.random.default_rng(6)
    corpus = unit_rows(rng, 40_000)
    corpus[123] *= np.float32(1e-33)      # norm far below fp32's comfortable range: no proven fp16 bound
    q = rng.standard_normal((8, 1024)).astype(np.float32)
    ix = _index(corpus, monkeypatch)
    try:
        got = ix.search(q, 10)
        assert "prefilter" not in ix.last_scan_kernel()
        want = oracle.exact_topk(q, corpus, 10, mode=oracle.F64, fast=True)
        assert_topk_matches(*got, *want, tol=TOL)
    finally:
        ix.close()



def test_workspace_state_is_left_clean_by_every_kind_of_search(gpu, monkeypatch):
    """The selection kernel zeroes its query's candidate count and class maxima when it is done with them, and the
    overflow word carries the sequence number of the search that overflowed (no kernel resets it).  A sequence of
    searches of different batch sizes on ONE workspace — plain, overflowing (answered by the fallback blocks of the
    selection launch), masked — must each give what a fresh index gives."""
    rng = np.random.default_rng(2024)
    n = 50_000
    corpus = unit_rows(rng, n)
    corpus[5_000:25_000] = corpus[3]                       # 20 000 duplicates: a query near row 3 overflows its list
    q_big = rng.standard_normal((64, 1024)).astype(np.float32)
    q_big -= np.outer(q_big @ corpus[3], corpus[3])        # these never near the duplicates
    q_over = np.concatenate([corpus[3][None] * 1.5, q_big[:6]])
    mask = rng.random(n) < 0.3
    packed = DenseIndex.pack_mask(mask)
    plan = [(q_big, None), (q_over, None), (q_big[:7], None), (q_over, packed), (q_big, packed), (q_big[:33], None),
            (q_over, None), (q_big, None)]
    ix = _index(corpus, monkeypatch)
    try:
        got = [ix.search(q, 10, row_mask=m) for q, m in plan]
    finally:
        ix.close()
    for (q, m), res in zip(plan, got):
        fresh = _index(corpus, monkeypatch)
        try:
            want = fresh.search(q, 10, row_mask=m)
        finally:
            fresh.close()
        for a, b in zip(res, want):
            assert np.array_equal(a, b, equal_nan=True)
    assert got[1][0][0].tolist() == [3] + list(range(5_000, 5_009))
    m8 = np.packbits(mask, bitorder="little")
    want = oracle.exact_topk(q_over[:2], corpus, 10, mask=m8, mode=oracle.F64, fast=True)
    assert_topk_matches(got[3][0][:2], got[3][1][:2], got[3][2][:2], *want, tol=TOL)


@pytest.mark.parametrize("k", [10, 100])
def test_a_search_that_fails_behind_its_scan_launch_leaves_no_stale_state(gpu, monkeypatch, k):
    """the selection kernel is what leaves a query's class maxima and candidate count zeroed, so a search
    that dies between its scan launch and its selection launch (an allocation failure, a launch error) leaves the
    scan's state in the workspace.  CRAG_TEST_FAIL_AFTER_SCAN=2 makes the second search return an error right
    there; its queries are copies of corpus rows (class maxima at 1.0), the next search's queries are random (best
    scores ~0.15): with stale maxima every true neighbour of the third search would be discarded.  The library marks
    the workspace dirty and re-zeroes it in front of the next search."""
    from cadence_rag_amd._native import NativeLibraryError as NativeError
    rng = np.random.default_rng(77)
    n = 48_000
    corpus = unit_rows(rng, n)
    q_plain = rng.standard_normal((64, 1024)).astype(np.float32)
    q_hot = corpus[rng.integers(0, n, size=64)].copy()
    monkeypatch.setenv("CRAG_TEST_FAIL_AFTER_SCAN", "2")
    ix = _index(corpus, monkeypatch)
    monkeypatch.delenv("CRAG_TEST_FAIL_AFTER_SCAN")
    try:
        first = ix.search(q_plain, k)
        assert "prefilter" in ix.last_scan_kernel()
        with pytest.raises(NativeError, match="injected failure"):
            ix.search(q_hot, k)
        third = ix.search(q_plain, k)
        fourth = ix.search(q_hot[:9], k)
    finally:
        ix.close()
    for a, b in zip(first, third):
        assert np.array_equal(a, b, equal_nan=True)
    want = oracle.exact_topk(q_plain[:4], corpus, k, mode=oracle.F64, fast=True)
    assert_topk_matches(third[0][:4], third[1][:4], third[2][:4], *want, tol=TOL)
    want = oracle.exact_topk(q_hot[:4], corpus, k, mode=oracle.F64, fast=True)
    assert_topk_matches(fourth[0][:4], fourth[1][:4], fourth[2][:4], *want, tol=TOL)


@pytest.mark.parametrize("n,nq,k", [(40_000, 1, 50), (60_000, 64, 100), (45_000, 7, 128), (50_000, 16, 33), (40_000, 130, 64)])
def test_selection_shared_by_several_blocks_per_query_equals_one_block(gpu, monkeypatch, n, nq, k):
    """k > 32: R = 4 or 8 selection blocks per query share the exact rescoring and the block that arrives last ranks
    their lists (CRAG_NO_RSPLIT=1: one block per query, round 2's form).  Same results bit for bit, the same rows
    rescored, also with a per-query mask and on repeated searches (the tickets are left at zero)."""
    rng = np.random.default_rng(n + nq + k)
    corpus = unit_rows(rng, n) * rng.uniform(0.1, 5.0, (n, 1)).astype(np.float32)
    q = rng.standard_normal((nq, 1024)).astype(np.float32)
    elig = rng.random((nq, n)) < 0.4
    packed = DenseIndex.pack_mask(elig)
    out = {}
    for split in (True, False):
        if split:
            monkeypatch.delenv("CRAG_NO_RSPLIT", raising=False)
        else:
            monkeypatch.setenv("CRAG_NO_RSPLIT", "1")
        ix = _index(corpus, monkeypatch)
        try:
            ix.prefilter_stats()
            res, stats = [], []
            for qq, m in ((q, None), (q, None), (q, packed), (q[: max(1, nq // 2)], None)):
                res.append(ix.search(qq, k, row_mask=m))
                stats.append(ix.prefilter_stats())   # per search (it synchronises and resets the sums)
            out[split] = (res, stats)
        finally:
            ix.close()
    monkeypatch.delenv("CRAG_NO_RSPLIT", raising=False)
    for a, b in zip(out[True][0], out[False][0]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    # the same searches took the selection path and the same rows were rescored (the number of CANDIDATES depends on when
    # the scan's workgroups saw each other's bounds: it varies from run to run, the survivors do not)
    # (a search whose candidate list overflows -- k = 128 on 45 000 rows can, depending on that timing -- is answered
    # by the fallback blocks and not counted: the results above are the same bits either way)
    may_overflow = (n, k) == (45_000, 128)
    for i, (a, b) in enumerate(zip(out[True][1], out[False][1])):
        assert a["searches"] <= 1 and b["searches"] <= 1
        if a["searches"] == b["searches"] == 1:
            assert a["rescored_rows"] == b["rescored_rows"], (i, a, b)
        elif not may_overflow:
            pytest.fail(f"search {i} went to the overflow fallback (R split: {a}, one block: {b})")
    s = min(nq, 3)
    want = oracle.exact_topk(q[:s], corpus, k, mode=oracle.F64, fast=True)
    got = out[True][0][0]
    assert_topk_matches(got[0][:s], got[1][:s], got[2][:s], *want, tol=TOL)


def test_hand_offs_under_load_four_streams_overflow_and_shared_selection(gpu, monkeypatch):
    """The two in-launch hand-offs of the selection kernel -- the fallback's "last block merges" and the R blocks per
    query of a large-k selection -- with the device busy: four streams launch overflowing searches, top-100 / top-50
    searches and plain ones back to back without synchronising.  Every answer equals the single-stream answer."""
    import torch
    rng = np.random.default_rng(31337)
    n = 60_000
    corpus = unit_rows(rng, n)
    corpus[8_000:30_000] = corpus[11]                    # 22 000 duplicates
    base = rng.standard_normal((64, 1024)).astype(np.float32)
    base -= np.outer(base @ corpus[11], corpus[11])
    jobs = [(np.concatenate([corpus[11][None] * 3.0, base[:9]]), 10),      # overflows -> fallback blocks
            (base, 10), (base[:7], 100), (base[:20], 50), (base[:33], 10), (base[:1], 64)]
    dev = torch.device("cuda", 0)
    ix = _index(corpus, monkeypatch)
    try:
        want = [ix.search(q, k) for q, k in jobs]
        assert want[0][0][0].tolist() == [11] + list(range(8_000, 8_009))
        streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
        dq = [torch.from_numpy(q).to(dev) for q, _ in jobs]
        torch.cuda.synchronize()
        outs = []
        for rep in range(6):
            for si, st in enumerate(streams):
                i = (si * 2 + rep) % len(jobs)
                nq, k = len(jobs[i][0]), jobs[i][1]
                o = (torch.empty(nq, k, dtype=torch.int64, device=dev), torch.empty(nq, k, dtype=torch.float32, device=dev),
                     torch.empty(nq, dtype=torch.int32, device=dev))
                ix.search_async(dq[i], k, *o, stream=st.cuda_stream)
                outs.append((i, o))
        torch.cuda.synchronize()
        for i, o in outs:
            assert np.array_equal(o[0].cpu().numpy(), want[i][0]), i
            assert np.array_equal(o[1].cpu().numpy(), want[i][1], equal_nan=True), i
            assert np.array_equal(o[2].cpu().numpy(), want[i][2]), i
    finally:
        ix.close()
