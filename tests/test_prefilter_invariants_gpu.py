"""The set of rows the prefilter path rescores exactly, checked on every search these tests issue.

Between prefilter_kernel (fp16 scan under a proven bound -> candidates) and finalize_fb_kernel (k-th approximate
score among the candidates -> cut -> exact rescoring) lies the candidate set, which the result comparisons alone do
not see: a candidate lost or staged twice outside the top-k of the compared queries changes no answer.  What does
show it is the number of rescored rows (prefilter_stats):

  * the selection rescores exactly the candidates whose approximate score is >= cut = trunc12(kth) - 2 PF_DELTA
    (kth: the k-th largest approximate score; trunc12 clears the FIN_SKIP_BITS low bits of its orderable form);
  * every row at or above kth - 2 PF_DELTA is a candidate, whatever the timing: it passes every threshold the scan
    can use (tau - 2 PF_DELTA with tau <= kth) and every re-test of a sift;
  * fewer than k eligible rows: no bound forms (the k_s-th largest class maximum of some set is empty), every
    eligible row is a candidate and the selection, with C <= k, rescores them all.

So the rescored count brackets against fp64 cosines (test a), and it is a function of (corpus, query, k, mask) only
-- the same under repeats, bound lags, cache policy, selection split, operand source, batching and streams (tests b,
c) -- PROVIDED no row's approximate score lies in [cut, kth - 2 PF_DELTA): a row there is a candidate only if it was
staged before the final bound arrived and was not re-tested since, which is timing.  The band is at most 2^-11 kth
wide (trunc12); the data of tests b and c are built with that band empty (_clear_band, from an fp16 model of the
approximate score), the bracket of test a holds either way.

Every invariant leg asserts that `searches` counts each search it issued: none of them went to the overflow
fallback, which answers without rescoring and without counting."""
import re
from pathlib import Path

import numpy as np
import pytest

from cadence_rag_amd.dense_index import DenseIndex
from tests.helpers import unit_rows

pytestmark = pytest.mark.gpu

_SRC = (Path(__file__).resolve().parent.parent / "cadence_rag_amd" / "csrc" / "crag_search.hip").read_text()


def _const(name):
    return re.search(rf"constexpr (?:int|float) {name} = ([0-9.e+-]+)f?;", _SRC).group(1)


PF_DELTA = float(np.float32(_const("PF_DELTA")))
FIN_SKIP_BITS = int(_const("FIN_SKIP_BITS"))
PF_FLUSH_ABOVE = int(_const("PF_FLUSH_ABOVE"))
PF_STASH = int(_const("PF_STASH_MIRROR"))
# The proven bound on |approximate score - cosine| (crag_search.hip, the comment under PF_DELTA): both unit operands
# rounded to fp16, (2u + u^2) sum|q_i c_i| <= 9.8e-4 (u = 2^-11, Cauchy-Schwarz); fp16 gradual underflow 1.9e-6;
# fp32 accumulation of 1024 products and 7 partial sums <= 1031 * 2^-23 = 1.23e-4; the fp32 normalisations
# 4 * 2^-24 and the fp32 chain vs the real cosine < 2e-6.  Sum 1.105e-3.
E = 1.105e-3
assert E < PF_DELTA
TRUNC_REL = 2.0 ** (FIN_SKIP_BITS - 23)   # clearing FIN_SKIP_BITS of a 23-bit mantissa: < 2^-11 relative


def _f2ord(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _ord2f(o):
    o = np.asarray(o, dtype=np.uint32)
    return np.where(o >> 31 == 1, o & np.uint32(0x7fffffff), ~o).astype(np.uint32).view(np.float32)


def _trunc(x):
    return _ord2f(_f2ord(x) & np.uint32((0xffffffff << FIN_SKIP_BITS) & 0xffffffff))


def _cosines(corpus, q):
    """fp64 cosines [nq, n] (NaN for a zero row)"""
    qn = q.astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True)
    out = np.empty((len(q), len(corpus)))
    for s in range(0, len(corpus), 16384):
        c = corpus[s:s + 16384].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            c /= np.linalg.norm(c, axis=1, keepdims=True)
        out[:, s:s + 16384] = qn @ c.T
    return out


def _approx(corpus, q):
    """A model of the scan's approximate score: both operands x fp32 1/norm, rounded to fp16, dot product (fp32 BLAS:
    within ~1e-6 of the MFMA's sum)"""
    def unit16(a):
        inv = (1.0 / np.linalg.norm(a.astype(np.float64), axis=1)).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            return (a * inv[:, None]).astype(np.float16).astype(np.float32)
    return unit16(q) @ unit16(corpus).T


def _eligible(n, nq, mask):
    if mask is None:
        return np.ones((nq, n), dtype=bool)
    return np.broadcast_to(mask, (nq, n))


def bracket(corpus, q, k, mask=None, cos=None):
    """(must, may) rescored rows per query from fp64 cosines"""
    cos = _cosines(corpus, q) if cos is None else cos
    elig = _eligible(len(corpus), len(q), mask) & np.isfinite(cos)
    must, may = [], []
    for i in range(len(q)):
        c = cos[i][elig[i]]
        if len(c) <= k:
            must.append(len(c))
            may.append(len(c))
            continue
        c64 = np.partition(c, len(c) - k)[len(c) - k]
        must.append(int(np.sum(c >= c64 - 2 * PF_DELTA + 2 * E)))
        may.append(int(np.sum(c >= c64 - 2 * PF_DELTA - 2 * E - TRUNC_REL * (abs(c64) + E) - 1e-6)))
    return np.array(must), np.array(may)


def _band_rows(corpus, q, k, mask):
    """per query: the eligible rows whose modelled approximate score lies in the timing band [cut, kth - 2 delta]
    (+- 2e-5 for the model)"""
    a = _approx(corpus, q)
    elig = _eligible(len(corpus), len(q), mask) & np.isfinite(a)
    out = []
    for i in range(len(q)):
        idx = np.nonzero(elig[i])[0]
        if len(idx) <= k:
            out.append(idx[:0])
            continue
        v = a[i, idx]
        kth = np.float32(np.partition(v, len(v) - k)[len(v) - k])
        lo = float(_trunc(np.float32(kth - 2e-5))) - 2 * PF_DELTA - 2e-5
        hi = float(kth) - 2 * PF_DELTA + 2e-5
        out.append(idx[(v >= lo) & (v <= hi)])
    return out


def _clear_band(rng, corpus, q, ks, mask=None):
    """Make the rescored set timing-independent for these queries and every k in ks: a row in some query's band is
    masked out for that query (per-query mask) or replaced by a fresh random row (cosine ~0 to everything, far
    below every band); neither changes a query's k-th score."""
    for _ in range(20):
        hit = False
        for k in ks:
            for i, rows in enumerate(_band_rows(corpus, q, k, mask)):
                if len(rows):
                    hit = True
                    if mask is not None and mask.ndim == 2:
                        mask[i, rows] = False
                    else:
                        norms = np.linalg.norm(corpus[rows], axis=1, keepdims=True)
                        corpus[rows] = unit_rows(rng, len(rows)) * norms
        if not hit:
            return
    raise AssertionError("could not clear the timing band")


def _index(corpus, monkeypatch, env=None):
    """a fresh index: the switches are read when it is created"""
    for key in ("CRAG_NO_PREFILTER", "CRAG_NO_RSPLIT", "CRAG_NO_FP16_MIRROR", "CRAG_PF_NT", "CRAG_PF_LAGS"):
        monkeypatch.delenv(key, raising=False)
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, v)
    ix = DenseIndex(corpus.shape[1], capacity=len(corpus))
    ix.add(corpus)
    for key in (env or {}):
        monkeypatch.delenv(key)
    return ix


def _counted(ix, q, k, packed=None, what=""):
    """one search + the statistics it alone produced; it may not have gone to the overflow fallback"""
    res = ix.search(q, k, row_mask=packed)
    assert "prefilter" in ix.last_scan_kernel(), ix.last_scan_kernel()
    s = ix.prefilter_stats()
    assert s["searches"] == 1, (what, s)
    return res, s["rescored_rows"]


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True), what


def _plain(corpus, q, k, monkeypatch, mask=None):
    """the plain fp32 scan's answer (CRAG_NO_PREFILTER=1)"""
    ix = _index(corpus, monkeypatch, {"CRAG_NO_PREFILTER": "1"})
    try:
        res = ix.search(q, k, row_mask=None if mask is None else DenseIndex.pack_mask(mask))
        assert "prefilter" not in ix.last_scan_kernel()
        return res
    finally:
        ix.close()


# ---- a. the bracket, query by query --------------------------------------------------------------------------------
def _near_tie_corpus(rng, n):
    """test_prefilter_gpu.test_dense_near_ties_stress_the_error_bound's construction: 6000 rows within a few 1e-4 of
    each other around the queries' k-th best, components pushed to the upper end of their fp16 rounding interval"""
    d = 1024
    base = rng.standard_normal(d).astype(np.float32)
    base /= np.linalg.norm(base)
    corpus = unit_rows(rng, n)
    cluster = base[None, :] + 2e-3 * rng.standard_normal((6000, d)).astype(np.float32)
    h = cluster.astype(np.float16).astype(np.float32)
    ulp = np.abs(np.spacing(cluster.astype(np.float16)).astype(np.float32))
    corpus[10_000:16_000] = (h + 0.499 * ulp * np.sign(h)).astype(np.float32)
    q = np.stack([base, base + 1e-3 * rng.standard_normal(d).astype(np.float32), -base])
    return corpus, q


KS = (1, 10, 32, 33, 64, 100, 128)


@pytest.mark.parametrize("kind", ["random", "near_ties", "mask_0.4", "mask_0.02", "fewer_than_k"])
def test_rescored_rows_lie_in_the_fp64_bracket(gpu, monkeypatch, kind):
    """Single-query searches (a per-query count): must <= rescored_rows <= may, for every k in KS, and the results
    are the plain fp32 scan's bit for bit."""
    rng = np.random.default_rng(sum(map(ord, kind)))
    n = 50_000
    mask = None
    if kind == "near_ties":
        corpus, q = _near_tie_corpus(rng, n)
    else:
        corpus = unit_rows(rng, n) * rng.uniform(0.2, 6.0, (n, 1)).astype(np.float32)
        q = rng.standard_normal((3, 1024)).astype(np.float32)
        if kind.startswith("mask"):
            mask = rng.random((len(q), n)) < float(kind.split("_")[1])
        elif kind == "fewer_than_k":
            mask = np.zeros((len(q), n), dtype=bool)
            for i, m in enumerate((5, 40, 100)):     # k in KS above and below each count
                mask[i, rng.choice(n, m, replace=False)] = True
    cos = _cosines(corpus, q)
    plain = _index(corpus, monkeypatch, {"CRAG_NO_PREFILTER": "1"})
    ix = _index(corpus, monkeypatch)
    try:
        for k in KS:
            must, may = bracket(corpus, q, k, mask, cos)
            for i in range(len(q)):
                packed = None if mask is None else DenseIndex.pack_mask(mask[i:i + 1])
                res, resc = _counted(ix, q[i:i + 1], k, packed)
                assert must[i] <= resc <= may[i], (kind, k, i, must[i], resc, may[i])
                if kind == "fewer_than_k" and mask[i].sum() <= k:
                    assert resc == mask[i].sum()
                _same(res, plain.search(q[i:i + 1], k, row_mask=packed), (kind, k, i))
    finally:
        ix.close()
        plain.close()


# ---- b. the same count under every change that must not matter ---------------------------------------------------
SETTINGS = [{}, {"CRAG_NO_RSPLIT": "1"}, {"CRAG_NO_FP16_MIRROR": "1"}, {"CRAG_PF_NT": "0"}, {"CRAG_PF_NT": "1"},
            {"CRAG_PF_LAGS": "1,2"}, {"CRAG_PF_LAGS": "2,4"}, {"CRAG_PF_LAGS": "3,4"}]


def _streams4(ix, q, k, mask):
    """the batch split in four, on four streams at once; the statistics of all four searches"""
    import torch
    dev = torch.device("cuda", 0)
    parts = np.array_split(np.arange(len(q)), 4)
    streams = [torch.cuda.Stream(device=dev) for _ in parts]
    outs = []
    for idx in parts:
        dq = torch.from_numpy(q[idx]).to(dev)
        o = (torch.empty(len(idx), k, dtype=torch.int64, device=dev), torch.empty(len(idx), k, device=dev),
             torch.empty(len(idx), dtype=torch.int32, device=dev))
        dm, stride = None, 0
        if mask is not None:
            pm = DenseIndex.pack_mask(mask[idx])
            dm, stride = torch.from_numpy(pm).to(dev), pm.shape[1]
        outs.append((dq, dm, stride, o))
    torch.cuda.synchronize()
    for st, (dq, dm, stride, o) in zip(streams, outs):   # back to back, nobody waits in between
        ix.search_async(dq, k, *o, d_row_mask=dm, mask_stride=stride, stream=st.cuda_stream)
    torch.cuda.synchronize()
    s = ix.prefilter_stats()
    assert s["searches"] == 4, s
    res = tuple(np.concatenate([o[j].cpu().numpy() for *_, o in outs]) for j in range(3))
    return res, s["rescored_rows"]


def _invariance_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    n, nq = 48_000, 64
    mask = None
    if name == "near_ties":
        corpus, q0 = _near_tie_corpus(rng, n)
        q = np.concatenate([q0, rng.standard_normal((nq - 3, 1024)).astype(np.float32)])
        k = 100
    else:
        corpus = unit_rows(rng, n) * rng.uniform(0.2, 6.0, (n, 1)).astype(np.float32)
        q = rng.standard_normal((nq, 1024)).astype(np.float32)
        k = 10 if name == "plain_k10" else 100
        if name == "mask_k100":
            mask = rng.random((nq, n)) < 0.4
    _clear_band(rng, corpus, q, (k,), mask)
    return corpus, q, k, mask


@pytest.mark.parametrize("name", ["plain_k10", "mask_k100", "near_ties"])
def test_rescored_rows_do_not_depend_on_timing_or_switches(gpu, monkeypatch, name):
    """Per case: the total rescored_rows and the results, bit for bit, are the same for 10 repeats, under each switch
    of SETTINGS (fresh index each), for the 64-query batch against its queries one at a time, and for the batch split
    across four concurrent streams -- and lie in the fp64 bracket."""
    corpus, q, k, mask = _invariance_case(name)
    packed = None if mask is None else DenseIndex.pack_mask(mask)
    must, may = bracket(corpus, q, k, mask)
    want = _plain(corpus, q, k, monkeypatch, mask)
    ref = None
    for env in SETTINGS:
        ix = _index(corpus, monkeypatch, env)
        try:
            ix.prefilter_stats()
            for rep in range(10 if not env else 2):
                res, resc = _counted(ix, q, k, packed, (env, rep))
                _same(res, want, (env, rep))
                ref = resc if ref is None else ref
                assert resc == ref, (env, rep, resc, ref)
            if not env:
                assert must.sum() <= ref <= may.sum(), (must.sum(), ref, may.sum())
                one = [_counted(ix, q[i:i + 1], k, None if mask is None else DenseIndex.pack_mask(mask[i:i + 1]))
                       for i in range(len(q))]
                assert sum(r for _, r in one) == ref
                for j in range(3):
                    assert np.array_equal(np.concatenate([o[j] for o, _ in one]), want[j], equal_nan=True)
                res, resc = _streams4(ix, q, k, mask)
                _same(res, want, "four streams")
                assert resc == ref
        finally:
            ix.close()


# ---- c. workloads that really sift ----------------------------------------------------------------------------------
def _wg_tiles(n, G):
    """prefilter_kernel's row ranges: workgroup g owns tiles [nt g / G, nt (g + 1) / G) of 32 rows"""
    nt = (n + 31) // 32
    return [(nt * g // G, nt * (g + 1) // G) for g in range(G)]


def _planted(rng, n, G, groups, masked):
    """Corpus with one planted cluster per query group: 3 full tiles of rows close to the group's base direction in
    the middle of one workgroup's range (>= PF_STASH tiles from either end: the first PF_STASH tiles in
    processing order are stashed, not staged, and a pass may run in reverse)."""
    corpus = unit_rows(rng, n)
    ranges = _wg_tiles(n, G)
    qs, masks, planted = [], [], []
    for gi, size in enumerate(groups):
        base = rng.standard_normal(1024).astype(np.float32)
        base /= np.linalg.norm(base)
        wg = (G // 3) * (gi + 1) + 1
        t0, t1 = ranges[wg]
        first = (t0 + (t1 - t0 - 3) // 2) * 32
        rows = np.arange(first, first + 96)
        assert first >= (t0 + PF_STASH) * 32 and first + 96 <= (t1 - PF_STASH) * 32, (t0, t1)
        corpus[rows] = base + 0.02 * rng.standard_normal((96, 1024)).astype(np.float32)
        qs.append(base + 0.02 * rng.standard_normal((size, 1024)).astype(np.float32))
        planted.append(rows)
    q = np.concatenate(qs)
    corpus *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    mask = None
    if masked:
        mask = rng.random((len(q), n)) < 0.5
        at = 0
        for size, rows in zip(groups, planted):
            mask[at:at + size, rows] = True
            at += size
    return corpus, q, mask, planted


@pytest.mark.parametrize("nq,masked", [(32, False), (32, True), (64, False), (64, True)])
def test_planted_clusters_force_flushing_sifts(gpu, monkeypatch, nq, masked):
    """Flush path by construction.  nq = 32 is one query block (NQB = 1), nq = 64 two (NQB = 2, one pass): every
    query of a group of 32 has the 96 planted rows of its group's workgroup far above its k-th best (cosine ~0.7 vs
    ~0.13) with k = 100 > 96, so every planted row is must-rescore and passes whatever threshold the scan has.  Each
    planted tile therefore stages 32 rows x 32 queries = 1024 > PF_FLUSH_ABOVE = 768 entries: at the next tile
    boundary the workgroup sifts, all 1024 survive (> 384 = PF_FLUSH_ABOVE / 2) and the sift flushes them to the
    global lists -- three flushes per planted workgroup (behind planted tiles 1, 2 and 3), with the other queries'
    staged candidates riding along.  A candidate lost or duplicated there changes rescored_rows and, being in the
    top-k, the results: both are checked against the plain fp32 scan, the fp64 bracket, and across repeats and
    switches."""
    assert 32 * 32 > PF_FLUSH_ABOVE and 32 * 32 > PF_FLUSH_ABOVE // 2
    rng = np.random.default_rng(nq + masked)
    n, k = 120_000, 100   # ~15 tiles per workgroup; candidates per query well below the cap of 8192
    probe = _index(np.ones((40_000, 1024), np.float32), monkeypatch)
    try:
        G = probe.scan_geometry(nq)["workgroups"]
    finally:
        probe.close()
    corpus, q, mask, planted = _planted(rng, n, G, [32] * (nq // 32), masked)
    _clear_band(rng, corpus, q, (k,), mask)
    cos = _cosines(corpus, q)
    must, may = bracket(corpus, q, k, mask, cos)
    for gi, rows in enumerate(planted):   # every planted row is must-rescore for its group
        sub = cos[32 * gi:32 * gi + 32]
        c = sub.copy()
        if mask is not None:
            c[~mask[32 * gi:32 * gi + 32]] = -np.inf
        kth = np.sort(c, axis=1)[:, -k]
        assert np.all(sub[:, rows].min(axis=1) >= kth - 2 * PF_DELTA + 2 * E)
        assert np.all(sub[:, rows].min(axis=1) > kth + 0.3)
    packed = None if mask is None else DenseIndex.pack_mask(mask)
    want = _plain(corpus, q, k, monkeypatch, mask)
    for gi, rows in enumerate(planted):
        assert set(rows.tolist()) <= set(want[0][32 * gi:32 * gi + 32].ravel().tolist())
    ref = None
    for env in ({}, {"CRAG_NO_RSPLIT": "1"}, {"CRAG_NO_FP16_MIRROR": "1"}, {"CRAG_PF_LAGS": "1,2"}):
        ix = _index(corpus, monkeypatch, env)
        try:
            ix.prefilter_stats()
            for rep in range(4):
                res, resc = _counted(ix, q, k, packed, (env, rep))
                _same(res, want, (env, rep))
                ref = resc if ref is None else ref
                assert resc == ref, (env, rep, resc, ref)
        finally:
            ix.close()
    assert must.sum() <= ref <= may.sum(), (must.sum(), ref, may.sum())


@pytest.mark.parametrize("n,nq,k", [(60_000, 64, 100), (52_000, 48, 120), (46_000, 33, 104)])
def test_small_corpus_large_k_keeps_its_rescored_set(gpu, monkeypatch, n, nq, k):
    """Where bounds form late and sifts that keep their survivors staged are common (the round-4 mismatch of the
    rescored count came from such a workload): per-query masks, rows of scaled norms.  Each case runs 28 times --
    twice under each switch of SETTINGS on one stream, and under the default and three of them split over four
    streams -- with the same rescored count and the plain scan's results every time."""
    rng = np.random.default_rng(n + nq + k)
    corpus = unit_rows(rng, n) * rng.uniform(0.05, 8.0, (n, 1)).astype(np.float32)
    q = rng.standard_normal((nq, 1024)).astype(np.float32)
    mask = rng.random((nq, n)) < rng.uniform(0.3, 0.9, (nq, 1))
    _clear_band(rng, corpus, q, (k,), mask)
    packed = DenseIndex.pack_mask(mask)
    must, may = bracket(corpus, q, k, mask)
    want = _plain(corpus, q, k, monkeypatch, mask)
    ref, runs = None, 0
    for env in SETTINGS:
        ix = _index(corpus, monkeypatch, env)
        try:
            ix.prefilter_stats()
            for rep in range(2):
                res, resc = _counted(ix, q, k, packed, (env, rep))
                _same(res, want, (env, rep))
                ref = resc if ref is None else ref
                assert resc == ref, (env, rep, resc, ref)
                runs += 1
            if env in ({}, {"CRAG_NO_RSPLIT": "1"}, {"CRAG_PF_LAGS": "1,2"}, {"CRAG_NO_FP16_MIRROR": "1"}):
                for rep in range(3):
                    res, resc = _streams4(ix, q, k, mask)
                    _same(res, want, (env, "four streams", rep))
                    assert resc == ref, (env, "four streams", rep, resc, ref)
                    runs += 1
        finally:
            ix.close()
    assert runs >= 25
    assert must.sum() <= ref <= may.sum(), (must.sum(), ref, may.sum())
