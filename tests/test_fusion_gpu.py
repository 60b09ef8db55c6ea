"""The three kernels every hybrid /retrieve answer leaves through -- rrf_fuse_kernel, tech_match_kernel +
tech_select_kernel, merge_results_kernel -- against tests/fusion_oracle.py at the edges of their code paths.

Rules of this file: every output is pre-filled with sentinels and carries one guard row past its end (padding is
asserted, an overrun is seen); every case runs twice and the two runs must be bit-equal; the comparison with the oracle
is exact (ids, counts, masks equal; scores equal as bit patterns, NaN pads included)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import fusion_oracle as fo
from cadence_rag_amd import _native, fusion
from cadence_rag_amd.dense_index import DenseIndex, ResultRecord

pytestmark = pytest.mark.gpu

SENT_ID = 0x5A5A5A5A5A5A5A5A
SENT_SCORE = 123.0
SENT_COUNT = -9
SENT_MASK = -1            # 0xFFFFFFFF in the int32 tensor the masks travel in
EINVAL = -1
CHUNK = 16384             # ranks per round of the token lane's selection


def _dev():
    return torch.device("cuda", 0)


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=_dev())


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _assert_sentinel(t, value, what):
    assert bool((t == value).all()), f"{what}: written where nothing may be written"


# =====================================================================================================
# reciprocal-rank fusion
# =====================================================================================================
def _fuse_outputs(nq, out_k):
    """Sentinel-filled outputs with one guard row."""
    return {"ids": _full((nq + 1, out_k), SENT_ID, torch.int64), "scores": _full((nq + 1, out_k), SENT_SCORE, torch.float64),
            "lanes": _full((nq + 1, out_k), SENT_MASK, torch.int32), "counts": _full((nq + 1,), SENT_COUNT, torch.int32)}


def _fuse_guard_intact(buf, nq):
    _assert_sentinel(buf["ids"][nq:], SENT_ID, "fused ids guard row")
    _assert_sentinel(buf["scores"][nq:], SENT_SCORE, "fused scores guard row")
    _assert_sentinel(buf["lanes"][nq:], SENT_MASK, "fused masks guard row")
    _assert_sentinel(buf["counts"][nq:], SENT_COUNT, "fused counts guard row")


def _fuse_raw(lib, lanes, widths, nq, rrf_k, out_k, buf, n_lanes=None):
    """crag_rrf_fuse itself, with whatever sizes the case names."""
    n = len(lanes)
    ids_arr = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t, _ in lanes])
    cnt_arr = (ctypes.c_void_p * max(n, 1))(*[c.data_ptr() for _, c in lanes])
    w_arr = (ctypes.c_int * max(n, 1))(*widths)
    rc = lib.crag_rrf_fuse(n if n_lanes is None else n_lanes, ids_arr, cnt_arr, w_arr, nq, rrf_k, out_k, _ptr(buf["ids"]),
                           _ptr(buf["scores"]), _ptr(buf["lanes"]), _ptr(buf["counts"]), None)
    torch.cuda.synchronize()
    return rc


def check_rrf(lanes_ids, lanes_counts, rrf_k, out_k):
    """lanes_ids[l] [nq, w_l] int64, lanes_counts[l] [nq]: fusion.rrf_fuse twice into sentinel-filled buffers == oracle."""
    nq = lanes_ids[0].shape[0]
    widths = [a.shape[1] for a in lanes_ids]
    lanes = [(_up(a.astype(np.int64)), _up(np.asarray(c, dtype=np.int32))) for a, c in zip(lanes_ids, lanes_counts)]
    runs = []
    for _ in range(2):
        buf = _fuse_outputs(nq, out_k)
        fusion.rrf_fuse(lanes, out_k, rrf_k, out={key: t[:nq] for key, t in buf.items()})
        torch.cuda.synchronize()
        _fuse_guard_intact(buf, nq)
        runs.append((buf["ids"][:nq].cpu().numpy(), buf["scores"][:nq].cpu().numpy().view(np.uint64),
                     buf["lanes"][:nq].cpu().numpy().view(np.uint32), buf["counts"][:nq].cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs of the same fusion differ"
    w_ids, w_sc, w_mask, w_ct = fo.rrf(lanes_ids, lanes_counts, widths, rrf_k, out_k)
    g_ids, g_sc, g_mask, g_ct = runs[0]
    assert np.array_equal(g_ct, w_ct), (g_ct, w_ct)
    bad = np.flatnonzero((g_ids != w_ids).any(axis=1))
    assert bad.size == 0, f"fused ids differ in queries {bad[:8]}: got {g_ids[bad[0]][:12]} want {w_ids[bad[0]][:12]}"
    assert np.array_equal(g_sc, w_sc.view(np.uint64)), "fused scores are not the Python floats bit for bit"
    assert np.array_equal(g_mask, w_mask)
    return w_ids, w_sc, w_mask, w_ct


def _split(total, n):
    """`total` as n non-negative widths; with three or more lanes one of them is 0."""
    if n == 1:
        return [total]
    live = n - 1 if n >= 3 else n
    base = [total // live + (1 if i < total % live else 0) for i in range(live)]
    if n >= 3:
        base.insert(1, 0)
    return base


def _lanes_with_totals(rng, widths, totals, pool_factor=1.5, garbage=True):
    """Per query q: counts that sum to totals[q] (each <= its width), keys without repeats inside a lane drawn from a
    pool small enough that lanes overlap; the cells behind a lane's count hold keys that must not be read."""
    nq = len(totals)
    ids = [np.empty((nq, w), dtype=np.int64) for w in widths]
    counts = [np.zeros(nq, dtype=np.int32) for _ in widths]
    for q, t in enumerate(totals):
        left = t
        for l in rng.permutation(len(widths)):               # a random share per lane ...
            c = int(rng.integers(0, min(widths[l], left) + 1))
            counts[l][q] = c
            left -= c
        for l in range(len(widths)):                         # ... and what is left over tops the lanes up in order
            add = min(widths[l] - counts[l][q], left)
            counts[l][q] += add
            left -= add
        assert left == 0 and sum(int(c[q]) for c in counts) == t
        pool = rng.permutation(max(int(t * pool_factor), max(widths) + 1)).astype(np.int64) * 7 + 3
        for l, w in enumerate(widths):
            ids[l][q] = rng.choice(pool, size=w, replace=False) if w else []
            if garbage:
                ids[l][q, counts[l][q]:] = 10 ** 9 + rng.integers(0, 50, size=w - counts[l][q])
    return ids, counts


TOTALS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024]


@pytest.mark.parametrize("n_lanes", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("rrf_k", [0, 1, 60])
def test_rrf_lane_counts_widths_and_totals(gpu, n_lanes, rrf_k):
    """1 to 8 lanes whose widths sum to exactly 1024 (one of width 0 from three lanes on); per-query totals on both
    sides of 4, 256 and 1024; out_k above and below the number of unique keys."""
    rng = np.random.default_rng(1000 + 10 * n_lanes + rrf_k)
    widths = _split(1024, n_lanes)
    assert sum(widths) == 1024 and (n_lanes < 3 or 0 in widths)
    ids, counts = _lanes_with_totals(rng, widths, TOTALS * 2)
    check_rrf(ids, counts, rrf_k, 1024)
    check_rrf(ids, counts, rrf_k, 200)      # the longer queries are cut, the shorter ones padded


def test_rrf_many_workgroups(gpu):
    rng = np.random.default_rng(7)
    ids, counts = _lanes_with_totals(rng, [50, 50, 100], rng.integers(0, 201, size=300).tolist())
    check_rrf(ids, counts, 60, 200)


def _with_repeats(rng, ids, counts, which):
    """Queries `which`: some cells of a lane overwritten with another cell of the same lane (an in-lane repeat)."""
    for q in which:
        for l in range(len(ids)):
            c = int(counts[l][q])
            if c >= 2:
                m = max(1, c // 4)
                dst, src = rng.integers(0, c, size=m), rng.integers(0, c, size=m)
                ids[l][q, dst] = ids[l][q, src]
    return ids


@pytest.mark.parametrize("dups", [False, True])
def test_rrf_cut_at_out_k(gpu, dups):
    """out_k in {1, unique-1, unique, unique+1, 1024, 1500} for a batch in which every query holds the same number of
    unique keys -- tied scores on both sides of every cut -- without and with repeats inside the lanes in every other
    query (the duplicate path is taken per workgroup)."""
    rng = np.random.default_rng(11 + dups)
    nq, unique = 96, 37
    keys = np.arange(unique, dtype=np.int64) * 5 + 2
    ids = [np.stack([rng.permutation(keys)[:w] for _ in range(nq)]) for w in (37, 20, 30)]
    counts = [np.full(nq, 37), rng.integers(0, 21, size=nq), rng.integers(0, 31, size=nq)]
    if dups:
        ids[1:] = _with_repeats(rng, ids[1:], counts[1:], range(0, nq, 2))      # lane 0 keeps all 37 keys
    for out_k in (1, unique - 1, unique, unique + 1, 1024, 1500):
        _, _, _, w_ct = check_rrf(ids, counts, 60, out_k)
        assert np.all(w_ct == min(unique, out_k))


def test_rrf_repeated_keys(gpu):
    """A key twice in one lane; the same key repeated in several lanes; a lane that is ONE key `width` times; queries
    with and without repeats in one batch; and repeats at the full 1024 items."""
    a = np.array([[1, 2, 1, 3], [1, 2, 4, 3], [5, 5, 5, 5], [9, 8, 7, 6]], dtype=np.int64)
    b = np.array([[4, 1, 1, 2], [3, 4, 2, 1], [5, 6, 5, 6], [6, 7, 8, 9]], dtype=np.int64)
    c = np.array([[7, 7, 7], [1, 5, 6], [5, 5, 5], [1, 2, 3]], dtype=np.int64)
    for rrf_k in (0, 60):
        w = check_rrf([a, b, c], [np.full(4, 4), np.full(4, 4), np.full(4, 3)], rrf_k, 11)
    assert w[0][2, :2].tolist() == [5, 6] and w[2][2, :2].tolist() == [7, 2]
    rng = np.random.default_rng(21)
    widths = [256, 256, 512]
    ids, counts = _lanes_with_totals(rng, widths, [1024, 1024, 1023, 700, 1024, 5], pool_factor=0.6)
    ids = _with_repeats(rng, ids, counts, [0, 2, 3, 5])
    ids[2][1, :] = 424242                                   # one key 512 times beside two ordinary lanes
    check_rrf(ids, counts, 60, 1024)
    check_rrf(ids, counts, 1, 100)


def test_rrf_counts_outside_the_lane_width(gpu):
    rng = np.random.default_rng(31)
    nq = 12
    ids = [rng.permutation(4000)[:nq * w].reshape(nq, w).astype(np.int64) + 10_000 * w for w in (6, 9, 4)]   # all distinct
    counts = [np.array([-1, -2 ** 31, 0, 6, 7, 11, 2 ** 31 - 1, 3, 6, 100, -7, 1]),
              np.array([9, 10, 2 ** 31 - 1, -3, 0, 9, 9, 5, 300, 9, 12, -1]),
              np.array([5, 4, 4, 2 ** 30, -2 ** 30, 0, 4, 4, 4, 1000, 3, 4])]
    w = check_rrf(ids, counts, 60, 19)
    assert w[3].tolist() == [13, 13, 13, 10, 6, 15, 19, 12, 19, 19, 12, 5]
    check_rrf(ids, counts, 0, 7)


def test_rrf_exact_ties_keep_first_insertion_order(gpu):
    """Keys that meet only at rank r of different lanes tie; so do keys whose sums run through the lanes crosswise
    (1/(k+1) + 1/(k+2) either way round).  The stable sort keeps the key inserted first in front -- neither the smaller
    id nor the later lane."""
    lane0 = np.array([[90, 10, 50, 3], [4, 5, 6, 7]], dtype=np.int64)
    lane1 = np.array([[80, 20, 40, 2], [5, 4, 7, 6]], dtype=np.int64)
    lane2 = np.array([[70, 30, 60, 1], [9, 9, 9, 9]], dtype=np.int64)
    for rrf_k in (0, 1, 60):
        ids, sc, _, ct = check_rrf([lane0, lane1, lane2], [np.full(2, 4), np.full(2, 4), np.array([4, 0])], rrf_k, 12)
        assert ids[0].tolist() == [90, 80, 70, 10, 20, 30, 50, 40, 60, 3, 2, 1]
        assert sc[0, 0] == sc[0, 1] == sc[0, 2] and sc[0, 3] == sc[0, 5]
        assert ids[1, :4].tolist() == [4, 5, 6, 7] and sc[1, 0] == sc[1, 1] and sc[1, 2] == sc[1, 3] and int(ct[1]) == 4
        cut = check_rrf([lane0, lane1, lane2], [np.full(2, 4), np.full(2, 4), np.array([4, 0])], rrf_k, 2)
        assert cut[0][0].tolist() == [90, 80] and cut[0][1].tolist() == [4, 5]


def test_rrf_probe_chain_of_1024_wraps_the_table_end(gpu):
    """1024 distinct keys that all hash to slot 2047 of the 2048-slot table: one chain that runs from the last slot
    through slot 0; then the same keys with repeats inside the lanes."""
    keys = fo.colliding_fuse_ids(2047, 1024)
    assert np.all(fo.fuse_slot(keys) == 2047) and np.unique(keys).size == 1024
    rng = np.random.default_rng(41)
    nq = 4
    perms = np.stack([rng.permutation(keys) for _ in range(nq)])
    ids = [perms[:, :256].copy(), perms[:, 256:512].copy(), perms[:, 512:].copy()]
    counts = [np.full(nq, 256), np.full(nq, 256), np.full(nq, 512)]
    _, _, _, ct = check_rrf(ids, counts, 60, 1024)
    assert np.all(ct == 1024)
    ids = _with_repeats(rng, ids, counts, [0, 2])
    ids[1][3, :100] = ids[0][3, :100][::-1]                 # query 3: keys shared by two lanes, no in-lane repeat
    check_rrf(ids, counts, 60, 1024)


def test_rrf_negative_and_very_large_ids(gpu):
    big = 2 ** 62
    lane0 = np.array([[-7, big, big - 1, 0, 2 ** 63 - 1]], dtype=np.int64)
    lane1 = np.array([[big + 1, -7, big, -2 ** 62, 5]], dtype=np.int64)
    ids, _, mask, ct = check_rrf([lane0, lane1], [np.array([5]), np.array([5])], 60, 9)
    assert int(ct[0]) == 8 and ids[0, 0] == -7 and int(mask[0, 0]) == 3


def test_rrf_abi_refusals_and_limits(gpu):
    """Every refusal comes back as CRAG_EINVAL before anything is launched (all pointers valid, the outputs keep their
    sentinels); a summed width of exactly 1024 is accepted; nq = 0 is CRAG_OK and launches nothing."""
    lib = gpu
    nq = 3
    lane = (_full((nq, 4), 5, torch.int64), _full((nq,), 4, torch.int32))
    wide = (_full((nq, 1024), 5, torch.int64), _full((nq,), 0, torch.int32))
    one = (_full((nq, 1), 6, torch.int64), _full((nq,), 1, torch.int32))

    def refused(lanes, widths, rrf_k, out_k, n_lanes=None, nq_=nq, rc_want=EINVAL):
        buf = _fuse_outputs(nq, max(out_k, 1))
        assert _fuse_raw(lib, lanes, widths, nq_, rrf_k, out_k, buf, n_lanes) == rc_want
        _fuse_guard_intact(buf, 0)                           # every row, not only the guard

    refused([lane] * 9, [4] * 9, 60, 8, n_lanes=0)
    refused([lane] * 9, [4] * 9, 60, 8, n_lanes=9)
    refused([lane], [4], 60, 0)
    refused([lane], [4], -1, 8)
    refused([wide, one], [1024, 1], 60, 8)
    assert "1024" in _native.last_error()
    refused([lane], [4], 60, 8, nq_=0, rc_want=0)
    buf = _fuse_outputs(nq, 8)
    assert _fuse_raw(lib, [wide], [1024], nq, 60, 8, buf) == 0          # summed width exactly 1024
    _fuse_guard_intact(buf, nq)
    assert buf["counts"][:nq].tolist() == [0, 0, 0] and bool((buf["ids"][:nq] == -1).all())
    assert _fuse_raw(lib, [lane] * 8, [4] * 8, nq, 60, 8, buf) == 0      # eight lanes
    assert buf["counts"][:nq].tolist() == [1, 1, 1] and buf["lanes"][0, 0].item() == 255


def test_hybrid_searcher_repads_its_reused_buffers(gpu):
    """HybridSearcher keeps the fused buffers per (stream, batch size, out_k): a second call with the same shape and far
    fewer hits must leave no row of the first call behind."""
    rng = np.random.default_rng(51)
    n, nq = 3000, 9
    corpus = rng.standard_normal((n, 1024)).astype(np.float32)
    row_tokens = [[f"T{int(t)}" for t in rng.integers(0, 20, size=rng.integers(0, 3))] for _ in range(n)]
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    started = np.datetime64("2026-01-01", "us") + rng.integers(0, 9, size=n).astype("timedelta64[D]")
    qv = _up(rng.standard_normal((nq, 1024)).astype(np.float32))
    qt = [[f"T{int(t)}" for t in rng.integers(0, 20, size=2)] for _ in range(nq)]
    few = np.zeros(n, dtype=bool)
    few[[5, 700, 2999]] = True
    masks = [None, _up(DenseIndex.pack_mask(few))]
    with DenseIndex(1024, capacity=n) as index:
        index.add(corpus, ids=ids)
        tech = fusion.TechTokenIndex(row_tokens, ids, started, _dev(), verify=False)
        hs = fusion.HybridSearcher(index, tech, dense_k=30, tech_k=20)
        seen = []
        for mask in masks + masks[1:]:
            out = hs.search(qv, qt, row_mask=mask)
            torch.cuda.synchronize()
            got = [out[key].cpu().numpy() for key in ("ids", "scores", "lanes", "counts")]
            t_ids, t_ct = (t.cpu().numpy() for t in tech.search(qt, 20, row_mask=mask, verify=False))
            lanes = [t_ids, out["dense_ids"].cpu().numpy()]
            lane_ct = [t_ct, out["dense_counts"].cpu().numpy()]
            w_ids, w_sc, w_mask, w_ct = fo.rrf(lanes, lane_ct, [20, 30], 60, 50)
            assert np.array_equal(got[3], w_ct) and np.array_equal(got[0], w_ids)
            assert np.array_equal(got[1].view(np.uint64), w_sc.view(np.uint64))
            assert np.array_equal(got[2].view(np.uint32), w_mask)
            seen.append((out["ids"].data_ptr(), got))
        assert seen[0][0] == seen[1][0] == seen[2][0]                    # the buffers really were reused
        assert int(seen[0][1][3].min()) >= 30 and int(seen[1][1][3].max()) <= 3
        for a, b in zip(seen[1][1], seen[2][1]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        tech.close()


# =====================================================================================================
# exact-token lane
# =====================================================================================================
def _csr(rows_by_rank):
    row_ptr = np.zeros(len(rows_by_rank) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows_by_rank], out=row_ptr[1:])
    flat = [t for r in rows_by_rank for t in r]
    return row_ptr, np.array(flat, dtype=np.uint64)


def _csr_random(rng, n, vocab, max_tok=3):
    """n rows of 0..max_tok tokens drawn from `vocab` (vectorised: the large cases have 100 000 rows)."""
    lens = rng.integers(0, max_tok + 1, size=n)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    return row_ptr, vocab[rng.integers(0, len(vocab), size=int(row_ptr[n]))]


def _queries(lists):
    qtok = np.zeros((len(lists), 32), dtype=np.uint64)
    for q, lst in enumerate(lists):
        qtok[q, :len(lst)] = lst
        qtok[q, len(lst):] = 0xDEAD0000 + q                 # behind the count: must not be read as tokens
    return qtok, np.array([len(lst) for lst in lists], dtype=np.int32)


def _mask(rng, kind, nq, n, density, extra=0):
    """(packed uint8 mask or None, mask_stride) over table POSITIONS."""
    if kind is None:
        return None, 0
    if kind == "shared":
        return DenseIndex.pack_mask(rng.random(max(n, 1)) < density)[:max((n + 31) // 32 * 4, 4)], 0
    packed = DenseIndex.pack_mask(rng.random((nq, max(n, 1))) < density)
    stride = (n + 31) // 32 * 4 + extra
    out = rng.integers(0, 256, size=(nq, max(stride, 4)), dtype=np.uint8)   # the slack between rows is noise
    out[:, :packed.shape[1]] = packed
    return out[:, :max(stride, 4)].copy() if stride else out, (stride if stride else 4)


def _tech_raw(lib, dev_args, n, nq, k, mask_t, stride, out_ids, out_ct, bitmap):
    order, row_ptr, toks, ids, qtok, qn = dev_args
    rc = lib.crag_tech_lane(_ptr(order), _ptr(row_ptr), _ptr(toks), None if ids is None else _ptr(ids), n, _ptr(qtok),
                            _ptr(qn), nq, k, None if mask_t is None else _ptr(mask_t), stride, _ptr(bitmap),
                            _ptr(out_ids), _ptr(out_ct), None)
    torch.cuda.synchronize()
    return rc


def _tech_device(order, row_ptr, toks, ids, qtok, qn):
    pad = lambda a, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(1, dtype=dt)])   # never an empty allocation
    return (_up(pad(order, np.int32)), _up(np.asarray(row_ptr, dtype=np.int64)), _up(pad(toks, np.uint64).view(np.int64)),
            None if ids is None else _up(pad(ids, np.int64)), _up(qtok.view(np.int64)), _up(qn))


def check_tech(lib, order, row_ptr, toks, ids, qtok, qn, k, mask=None, stride=0, dev_args=None):
    """crag_tech_lane on device tensors built here, twice, into sentinel-filled outputs == oracle."""
    n, nq = len(order), qtok.shape[0]
    dev_args = dev_args or _tech_device(order, row_ptr, toks, ids, qtok, qn)
    mask_t = None if mask is None else _up(mask)
    words = max(1, (n + 63) // 64)
    runs = []
    for rep in range(2):
        out_ids, out_ct = _full((nq + 1, k), SENT_ID, torch.int64), _full((nq + 1,), SENT_COUNT, torch.int32)
        bitmap = _full((words * nq + 64,), 0x7777777777777777 if rep else -1, torch.int64)   # scratch: stale bits
        assert _tech_raw(lib, dev_args, n, nq, k, mask_t, stride, out_ids, out_ct, bitmap) == 0, _native.last_error()
        _assert_sentinel(out_ids[nq:], SENT_ID, "token lane ids guard row")
        _assert_sentinel(out_ct[nq:], SENT_COUNT, "token lane counts guard row")
        _assert_sentinel(bitmap[words * nq:], 0x7777777777777777 if rep else -1, "bitmap scratch guard")
        runs.append((out_ids[:nq].cpu().numpy(), out_ct[:nq].cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs differ"
    w_ids, w_ct = fo.tech_lane(order, row_ptr, toks, ids, qtok, qn, k, mask, stride)
    assert np.array_equal(runs[0][1], w_ct), (runs[0][1], w_ct)
    bad = np.flatnonzero((runs[0][0] != w_ids).any(axis=1))
    assert bad.size == 0, f"token lane ids differ in queries {bad[:8]}"
    return w_ids, w_ct


_NQ_OF = {0: 37, 1: 64, 63: 1, 64: 63, 65: 37, CHUNK - 1: 64, CHUNK: 1, CHUNK + 1: 63, 2 * CHUNK + 70: 37, 100_000: 64}
MASKS = [(None, 0.0, 0), ("shared", 0.5, 0), ("per", 0.5, 0), ("per", 0.01, 12), ("per", 0.0, 0), ("shared", 1.0, 0),
         ("per", 1.0, 4), ("shared", 0.01, 0)]


@pytest.mark.parametrize("n", sorted(_NQ_OF))
def test_tech_lane_row_counts_and_masks(gpu, n):
    """n on both sides of a 64-rank word and of a 16 384-rank chunk, down to 0; nq in {1, 37, 63, 64}; rows of 0, 1, a
    few and 40 tokens, rows whose tokens all miss, hashes 0 and 1 on both sides; no mask, a shared mask, per-query masks
    at the minimal and at a larger stride, densities 0 / 0.01 / 0.5 / 1; with and without external ids."""
    rng = np.random.default_rng(2000 + n % 997)
    nq = _NQ_OF[n]
    vocab = np.concatenate([np.array([0, 1], dtype=np.uint64), rng.integers(2, 2 ** 63, size=198).astype(np.uint64) * 2 + 1])
    strangers = rng.integers(2, 2 ** 63, size=300).astype(np.uint64) * 2        # even: never a query token
    both = np.concatenate([vocab, strangers])
    row_ptr, toks = _csr_random(rng, n, both)
    if n >= 63:                                              # a few rows of 40 tokens, among them only strangers
        rows = [toks[row_ptr[r]:row_ptr[r + 1]].tolist() for r in range(n)] if n <= 65 else None
        if rows is not None:
            rows[3] = rng.choice(both, size=40, replace=False).tolist()
            rows[n - 1] = rng.choice(strangers, size=40, replace=False).tolist()
            rows[n - 2] = [int(vocab[5])] * 40
            row_ptr, toks = _csr(rows)
    order = rng.permutation(n).astype(np.int32)
    ids = rng.permutation(max(n, 1))[:n].astype(np.int64) * 3 - 7
    lists = [rng.choice(vocab, size=int(m), replace=False).tolist() for m in rng.integers(0, 6, size=nq)]
    lists[0] = rng.choice(vocab, size=32, replace=False).tolist()
    if nq > 2:
        lists[1], lists[2] = [0], [1]
    qtok, qn = _queries(lists)
    dev_args = _tech_device(order, row_ptr, toks, ids, qtok, qn)
    masks = MASKS if n < 100_000 else [MASKS[0], MASKS[2]]
    for i, (kind, density, extra) in enumerate(masks):
        mask, stride = _mask(rng, kind, nq, n, density, extra)
        k = [1, 7, 50, 128, max(n, 1), n + 5][i % 6] if n < 100_000 else 50
        check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, k, mask, stride, dev_args=dev_args)
    if n < 100_000:
        check_tech(gpu, order, row_ptr, toks, None, qtok, qn, 33, *_mask(rng, "per", nq, n, 0.5, 8))   # ids = NULL


def test_tech_lane_limit_k_inside_a_word_and_at_the_chunk_boundary(gpu):
    """Every row matches every query (a token all 64 queries share): the first k ranks are the answer, for k around a
    64-rank word, around the 16 384-rank chunk, n and n + 5; then under per-query masks, where the cut falls at a
    different rank for every query."""
    rng = np.random.default_rng(61)
    n = 2 * CHUNK + 70
    shared = np.uint64(0xABCDEF0123456789)
    lens = rng.integers(1, 4, size=n)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    toks = rng.integers(2, 2 ** 62, size=int(row_ptr[n])).astype(np.uint64)
    toks[row_ptr[:-1] + rng.integers(0, 4, size=n) % lens] = shared
    order = rng.permutation(n).astype(np.int32)
    ids = np.arange(n, dtype=np.int64) + 1000
    for nq, ks in ((64, (1, 63, 64, 65)), (37, (CHUNK - 1, CHUNK, CHUNK + 1)), (2, (n, n + 5))):
        lists = [[int(shared)] + rng.integers(2, 2 ** 62, size=int(rng.integers(0, 31))).tolist() for _ in range(nq)]
        qtok, qn = _queries(lists)
        dev_args = _tech_device(order, row_ptr, toks, ids, qtok, qn)
        half, stride = _mask(rng, "per", nq, n, 0.5, 0)
        for k in ks:
            w_ids, w_ct = check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, k, dev_args=dev_args)
            assert np.all(w_ct == min(k, n)) and np.array_equal(w_ids[0, :min(k, n)], ids[order[:min(k, n)]])
            if k < n:
                check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, k, half, stride, dev_args=dev_args)


def test_tech_lane_sparse_matches_reach_k_in_the_third_chunk(gpu):
    rng = np.random.default_rng(62)
    n, nq, k = 2 * CHUNK + 70, 5, 25
    wanted = np.array([11, 12, 13, 14, 15], dtype=np.uint64)
    rows = [[int(1000 + r)] for r in range(n)]
    for q in range(nq):
        hit = np.concatenate([rng.choice(CHUNK, 9, replace=False), CHUNK + rng.choice(CHUNK, 9, replace=False),
                              2 * CHUNK + rng.choice(70, 20, replace=False)])
        for r in hit:
            rows[r] = rows[r] + [int(wanted[q])]
    rows[2 * CHUNK + 69].append(int(wanted[0]))                        # the very last rank
    row_ptr, toks = _csr(rows)
    qtok, qn = _queries([[int(w)] for w in wanted])
    order = rng.permutation(n).astype(np.int32)
    for kk in (k, 18, 19, 60):
        _, w_ct = check_tech(gpu, order, row_ptr, toks, None, qtok, qn, kk)
    assert w_ct.max() <= 39 and w_ct.min() >= 38


def test_tech_lane_hashes_zero_and_one_are_one_token(gpu):
    rows = [[0], [1], [0, 1], [2], [], [5, 0], [1, 5], [3], [0] * 40, [7] * 40]
    row_ptr, toks = _csr(rows)
    order = np.arange(len(rows), dtype=np.int32)[::-1].copy()
    qtok, qn = _queries([[0], [1], [0, 1], [2], [], [1, 0, 1, 0], [3, 0]])
    w_ids, w_ct = check_tech(gpu, order, row_ptr, toks, None, qtok, qn, 10)
    assert w_ct.tolist() == [6, 6, 6, 1, 0, 6, 7] and w_ids[0, :6].tolist() == w_ids[1, :6].tolist()


def test_tech_lane_hash_zero_through_the_host_entry(gpu, monkeypatch):
    """TechTokenIndex with a token_hash that gives 0 and 1: hash 0 reaches crag_tech_lane_host on both sides."""
    real = fusion.token_hash
    fake = lambda t: {"ZERO": 0, "ONE": 1}.get(t, real(t))
    monkeypatch.setattr(fusion, "token_hash", fake)
    fusion._hash_cache.clear()
    rng = np.random.default_rng(63)
    n = 500
    vocab = ["ZERO", "ONE", "A", "B", "C", "D"]
    row_tokens = [list(rng.choice(vocab, size=int(rng.integers(0, 3)), replace=False)) for _ in range(n)]
    ids = np.arange(n, dtype=np.int64) + 40
    started = np.datetime64("2026-02-01", "us") + rng.integers(0, 9, size=n).astype("timedelta64[D]")
    queries = [["ZERO"], ["ONE"], ["ZERO", "ONE"], ["A"], ["A", "ZERO"], []]
    tech = fusion.TechTokenIndex(row_tokens, ids, started, _dev(), verify=False)
    try:
        order = np.lexsort((ids, -started.astype(np.int64))).astype(np.int32)
        row_ptr, toks = _csr([[fake(t) for t in row_tokens[p]] for p in order])
        qtok, qn = _queries([[fake(t) for t in q] for q in queries])
        elig = rng.random(n) < 0.5
        for mask in (None, DenseIndex.pack_mask(elig)):
            w_ids, w_ct = fo.tech_lane(order, row_ptr, toks, ids, qtok, qn, 30, mask, 0)
            runs = []
            for _ in range(2):
                g_ids, g_ct = tech.search(queries, 30, row_mask=None if mask is None else _up(mask), verify=False)
                torch.cuda.synchronize()
                runs.append((g_ids.cpu().numpy(), g_ct.cpu().numpy()))
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
            assert np.array_equal(runs[0][1], w_ct) and np.array_equal(runs[0][0], w_ids)
        assert np.array_equal(w_ids[0], w_ids[1])
    finally:
        tech.close()
        fusion._hash_cache.clear()


def test_tech_lane_full_query_table(gpu):
    """64 queries x 32 distinct tokens: all 2048 entries of the table, bit 63 of the query set (query 63 is the only
    owner of its tokens), beside tokens that all 64 queries share."""
    rng = np.random.default_rng(64)
    n, nq = 3000, 64
    uniq = (rng.permutation(1 << 20)[:nq * 32].astype(np.uint64) << np.uint64(40)) + np.uint64(12345)
    lists = uniq.reshape(nq, 32).tolist()
    qtok, qn = _queries(lists)
    strangers = rng.integers(2, 2 ** 40, size=100).astype(np.uint64)
    row_ptr, toks = _csr_random(rng, n, np.concatenate([uniq, strangers]), max_tok=2)
    last = np.flatnonzero(np.isin(toks, uniq[63 * 32:]))
    assert last.size > 20                                               # query 63 has rows of its own
    order = rng.permutation(n).astype(np.int32)
    ids = np.arange(n, dtype=np.int64) * 2
    for kind, density, extra in MASKS[:4]:
        w_ids, w_ct = check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, 40, *_mask(rng, kind, nq, n, density, extra))
    common = uniq[:31].tolist()                                         # 31 tokens in every query + one of its own
    qtok, qn = _queries([common + [int(uniq[100 + q])] for q in range(nq)])
    _, w_ct = check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, 25)
    assert np.all(w_ct == 25)
    check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, 64, *_mask(rng, "per", nq, n, 0.5, 4))


def test_tech_lane_probe_chain_of_2048_wraps_the_table_end(gpu):
    """2048 query tokens that all hash to slot 4095 of the 4096-slot table -- one chain from the last slot through
    slot 0 -- and rows that hold members and colliding non-members (every miss walks the whole chain)."""
    rng = np.random.default_rng(65)
    n, nq = 1500, 64
    hs = fo.colliding_tech_hashes(4095, 2048 + 200)
    assert np.all(fo.tech_slot(hs) == 4095)
    hs = rng.permutation(hs)
    members = hs[:2048]
    qtok, qn = _queries(members.reshape(nq, 32).tolist())
    row_ptr, toks = _csr_random(rng, n, hs, max_tok=3)
    order = rng.permutation(n).astype(np.int32)
    ids = np.arange(n, dtype=np.int64) + 9
    for kind, density, extra in (MASKS[0], MASKS[2], MASKS[3]):
        _, w_ct = check_tech(gpu, order, row_ptr, toks, ids, qtok, qn, 50, *_mask(rng, kind, nq, n, density, extra))
    assert w_ct.max() > 0


def test_tech_lane_refuses_a_bad_mask_stride(gpu):
    """With a mask, mask_stride is 0 or a multiple of 4 of at least ceil(n/32)*4 bytes: anything else used to be divided
    by 4 and read the wrong words.  Refused with CRAG_EINVAL before any launch, through both entries."""
    lib = gpu
    n, nq, k = 200, 4, 5
    order = np.arange(n, dtype=np.int32)
    row_ptr, toks = _csr([[7]] * n)
    qtok, qn = _queries([[7]] * nq)
    dev_args = _tech_device(order, row_ptr, toks, None, qtok, qn)
    mask_t = _full((nq * 64,), 0xFF, torch.uint8)                       # large enough for every stride tried
    need = (n + 31) // 32 * 4
    out_ids, out_ct = _full((nq + 1, k), SENT_ID, torch.int64), _full((nq + 1,), SENT_COUNT, torch.int32)
    bitmap = _full((4 * nq,), -1, torch.int64)
    for stride in (6, need - 4, need + 2, 4, -4):
        assert _tech_raw(lib, dev_args, n, nq, k, mask_t, stride, out_ids, out_ct, bitmap) == EINVAL, stride
        assert "mask_stride" in _native.last_error()
        _assert_sentinel(out_ids, SENT_ID, "ids after a refusal")
        _assert_sentinel(out_ct, SENT_COUNT, "counts after a refusal")
        _assert_sentinel(bitmap, -1, "scratch after a refusal")
    slot = lib.crag_upload_slot_create()
    assert slot
    try:
        h_tok = (ctypes.c_uint64 * nq)(*[7] * nq)
        h_cnt = (ctypes.c_int32 * nq)(*[1] * nq)
        order_t, row_ptr_t, toks_t = dev_args[:3]
        for stride, want in ((6, EINVAL), (need - 4, EINVAL), (need, 0), (0, 0)):
            rc = lib.crag_tech_lane_host(_ptr(order_t), _ptr(row_ptr_t), _ptr(toks_t), None, n, h_tok, h_cnt, nq, k,
                                         _ptr(mask_t), stride, slot, _ptr(bitmap), _ptr(out_ids), _ptr(out_ct), None)
            torch.cuda.synchronize()
            assert rc == want, (stride, _native.last_error())
            if want:
                _assert_sentinel(out_ids, SENT_ID, "ids after a refused host call")
        assert out_ct[:nq].tolist() == [k] * nq and out_ids[0].tolist() == [0, 1, 2, 3, 4]
        _assert_sentinel(out_ids[nq:], SENT_ID, "guard row")
    finally:
        lib.crag_upload_slot_destroy(slot)
    assert _tech_raw(lib, dev_args, n, nq, k, None, 6, out_ids, out_ct, bitmap) == 0     # no mask: the stride is unused


# =====================================================================================================
# cross-shard merge
# =====================================================================================================
def _sorted_lists(rng, n_lists, nq, k, values, counts):
    """Per (list, query): `k` scores drawn from `values`, sorted as a search leaves them (ordered bits descending, then
    id ascending); ids unique per query over all lists (shards are disjoint); the cells behind a list's count hold
    values that must be dropped."""
    sc = rng.choice(np.asarray(values, dtype=np.float32), size=(n_lists, nq, k))
    ids = np.empty((n_lists, nq, k), dtype=np.int64)
    for q in range(nq):
        ids[:, q, :] = (rng.permutation(n_lists * k).astype(np.int64) * 11 - 5).reshape(n_lists, k)
    ob = fo.ordered_bits(sc).astype(np.int64)
    idx = np.lexsort((ids, -ob), axis=2)
    sc, ids = np.take_along_axis(sc, idx, axis=2), np.take_along_axis(ids, idx, axis=2)
    behind = np.arange(k)[None, None, :] >= np.asarray(counts)[:, :, None]
    sc[behind] = np.float32(np.inf)
    ids[behind] = 777_777_777
    return ids, sc


def check_merge(lib, ids, sc, ct, k):
    """crag_merge_topk and crag_merge_topk_packed (records assembled from the same arrays), each twice: same bits as
    each other and as the oracle."""
    n_lists, nq, _ = ids.shape
    ct = np.asarray(ct, dtype=np.int32)
    rec = ResultRecord.record_bytes(nq, k)
    raw = np.full((n_lists, rec), 0xEE, dtype=np.uint8)
    raw[:, :nq * k * 8] = ids.reshape(n_lists, -1).view(np.uint8)
    raw[:, nq * k * 8:nq * k * 12] = sc.reshape(n_lists, -1).view(np.uint8)
    raw[:, nq * k * 12:nq * k * 12 + nq * 4] = ct.view(np.uint8).reshape(n_lists, -1)
    d_ids, d_sc, d_ct, d_rec = _up(ids), _up(sc), _up(ct), _up(raw)
    runs = []
    for entry in ("arrays", "packed", "arrays", "packed"):
        o_ids, o_sc = _full((nq + 1, k), SENT_ID, torch.int64), _full((nq + 1, k), SENT_SCORE, torch.float32)
        o_ct = _full((nq + 1,), SENT_COUNT, torch.int32)
        if entry == "arrays":
            rc = lib.crag_merge_topk(0, _ptr(d_ids), _ptr(d_sc), _ptr(d_ct), n_lists, nq, k, _ptr(o_ids), _ptr(o_sc),
                                     _ptr(o_ct), None)
        else:
            rc = lib.crag_merge_topk_packed(0, _ptr(d_rec), n_lists, nq, k, _ptr(o_ids), _ptr(o_sc), _ptr(o_ct), None)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        _assert_sentinel(o_ids[nq:], SENT_ID, "merged ids guard row")
        _assert_sentinel(o_sc[nq:], SENT_SCORE, "merged scores guard row")
        _assert_sentinel(o_ct[nq:], SENT_COUNT, "merged counts guard row")
        runs.append((o_ids[:nq].cpu().numpy(), o_sc[:nq].cpu().numpy().view(np.uint32), o_ct[:nq].cpu().numpy()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b), "the two entries, or two runs of one, differ"
    w_ids, w_sc, w_ct = fo.merge(ids, sc, ct, k)
    assert np.array_equal(runs[0][2], w_ct), (runs[0][2], w_ct)
    assert np.array_equal(runs[0][0], w_ids)
    assert np.array_equal(runs[0][1], w_sc.view(np.uint32))
    return w_ids, w_sc, w_ct


MERGE_SHAPES = [(1, 5, 1), (1, 3, 128), (2, 64, 100), (32, 7, 128), (4096, 2, 1)]


@pytest.mark.parametrize("n_lists,nq,k", MERGE_SHAPES)
def test_merge_shapes_counts_signs_and_ties(gpu, n_lists, nq, k):
    """One list, k = 1, n_lists * k = 4096 (the LDS capacity); random counts, all zero, mixed 0 and k; negative scores;
    a handful of score values spread over all lists, so that the id decides across many lists; +0.0 beside -0.0."""
    rng = np.random.default_rng(3000 + n_lists + k)
    spread = rng.standard_normal(4000).astype(np.float32)
    few = np.array([0.75, 0.5, -0.25, -1.5], dtype=np.float32)
    zeros = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    full = np.full((n_lists, nq), k)
    cases = [(spread, rng.integers(0, k + 1, size=(n_lists, nq))), (spread, full), (spread, np.zeros((n_lists, nq), dtype=int)),
             (spread, k * rng.integers(0, 2, size=(n_lists, nq))), (-np.abs(spread) - 1, full), (few, full),
             (few[:1], rng.integers(0, k + 1, size=(n_lists, nq))), (zeros, full), (zeros[:2], full)]
    for values, counts in cases:
        ids, sc = _sorted_lists(rng, n_lists, nq, k, values, counts)
        w_ids, w_sc, w_ct = check_merge(gpu, ids, sc, counts, k)
        assert np.array_equal(w_ct, np.minimum(np.asarray(counts).sum(axis=0), k))
    plus = (sc.view(np.uint32) == 0).any(axis=(0, 2))                       # the last case: a +0.0 leads, whatever the ids
    assert np.all(w_ct == k) and np.array_equal(w_sc.view(np.uint32)[:, 0] == 0, plus)


def test_merge_one_score_in_five_lists_the_id_decides(gpu):
    ids = np.array([[[50, 60]], [[10, 70]], [[40, 45]], [[5, 90]], [[30, 31]]], dtype=np.int64)
    sc = np.full((5, 1, 2), 0.5, dtype=np.float32)
    sc[3, 0, 1] = 0.25
    w_ids, _, _ = check_merge(gpu, ids, sc, np.full((5, 1), 2), 2)
    assert w_ids[0].tolist() == [5, 10]
    ct = np.array([[2], [0], [2], [1], [2]])
    assert check_merge(gpu, ids, sc, ct, 2)[0][0].tolist() == [5, 30]


def test_merge_refuses_more_than_4096_candidates(gpu):
    lib = gpu
    n_lists, nq, k = 4097, 2, 1
    ids, sc = _full((n_lists, nq, k), 3, torch.int64), _full((n_lists, nq, k), 0.5, torch.float32)
    ct = _full((n_lists, nq), 1, torch.int32)
    rec = _full((n_lists * ResultRecord.record_bytes(nq, k),), 0, torch.uint8)
    o_ids, o_sc, o_ct = _full((nq + 1, k), SENT_ID, torch.int64), _full((nq + 1, k), SENT_SCORE, torch.float32), \
        _full((nq + 1,), SENT_COUNT, torch.int32)
    assert lib.crag_merge_topk(0, _ptr(ids), _ptr(sc), _ptr(ct), n_lists, nq, k, _ptr(o_ids), _ptr(o_sc), _ptr(o_ct),
                               None) == EINVAL
    assert "4096" in _native.last_error()
    assert lib.crag_merge_topk_packed(0, _ptr(rec), n_lists, nq, k, _ptr(o_ids), _ptr(o_sc), _ptr(o_ct), None) == EINVAL
    assert lib.crag_merge_topk(0, _ptr(ids), _ptr(sc), _ptr(ct), 33, nq, 128, _ptr(o_ids), _ptr(o_sc), _ptr(o_ct),
                               None) == EINVAL                            # 33 * 128 = 4224 (never launched)
    torch.cuda.synchronize()
    _assert_sentinel(o_ids, SENT_ID, "ids after a refusal")
    _assert_sentinel(o_sc, SENT_SCORE, "scores after a refusal")
    _assert_sentinel(o_ct, SENT_COUNT, "counts after a refusal")
