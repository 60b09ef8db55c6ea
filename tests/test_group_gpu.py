"""The grouped search (crag_index_search_grouped_async) on the GPU, with no tolerance anywhere: the reference values are the
lane's own scores -- the per-slot scores of crag_index_search_ids_async over every stored id, which are the bits of the
masked search -- walked by the numpy oracle (tests/group_oracle.py); ids, score bits, groups and counts must be equal.
Then equality with crag_index_search itself where the cap cannot bind, ties, the order in which keys reach a group's
slots, determinism on a dirty scratch, a slot table larger than the select kernel's LDS buffer, edits, the optional
output, and the route through DenseTable / GpuRetrieveBackend / the DENSE_PER_CALL_CAP knob."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from cadence_rag_amd import _native
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.config import settings
from cadence_rag_amd.dense_index import DenseIndex
from group_oracle import capped_topk

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N_ROWS = 200          # three full workgroups of the score kernel (64 positions each) and a ragged fourth
N_GROUPS = 23
Q_BLOCK = 16          # queries the score kernel holds in LDS at a time (GQ_BLOCK of csrc/crag_group.hip)
KS = (1, 32, 33, 128)
PERS = (1, 2, 3, 8)
NQS = (1, 3, Q_BLOCK + 1, 64)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Data:
    """n rows, ids 10 + 3 * position, 23 groups dealt out by a permutation (no group is contiguous): group 0 holds one
    row, group 1 none, group 2 twelve (more than CRAG_GROUP_MAX_PER); one row is numbered -1 and one n_groups.  A twin
    pair inside group 2, a twin pair across groups 3 and 4, a zero row and a NaN row."""

    def __init__(self, n: int, dim: int, seed: int) -> None:
        rng = np.random.default_rng(seed)
        rows = rng.standard_normal((n, dim)).astype(np.float32) * rng.uniform(0.2, 5.0, size=(n, 1)).astype(np.float32)
        perm = rng.permutation(n)
        groups = np.empty(n, dtype=np.int32)
        groups[perm[0]] = 0
        groups[perm[1:13]] = 2
        groups[perm[13]] = -1
        groups[perm[14]] = N_GROUPS
        groups[perm[15:]] = 3 + np.arange(n - 15) % (N_GROUPS - 3)
        self.inside = tuple(sorted(int(p) for p in perm[1:3]))                          # twins inside group 2
        self.across = tuple(sorted((int(perm[15]), int(perm[16]))))                     # twins in groups 3 and 4
        self.zero_pos, self.nan_pos = int(perm[17]), int(perm[18])
        rows[self.inside[1]] = rows[self.inside[0]]
        rows[self.across[1]] = rows[self.across[0]]
        rows[self.zero_pos] = 0.0
        rows[self.nan_pos, dim // 2] = np.nan
        self.rows, self.n, self.dim, self.rng, self.groups = rows, n, dim, rng, groups
        self.ids = 10 + 3 * np.arange(n, dtype=np.int64)
        assert sorted(np.bincount(groups[(groups >= 0) & (groups < N_GROUPS)], minlength=N_GROUPS)[:3].tolist()) == [0, 1, 12]
        q = rng.standard_normal((64, dim)).astype(np.float32)
        q[0] = rows[self.inside[0]] * 0.5                 # the twins of group 2 tie at the top of query 0
        q[1] = 0.0                                        # a zero query
        q[2, 0] = np.nan                                  # a non-finite query
        q[3] = rows[self.across[0]] * 0.7                 # the twins of groups 3 / 4 tie at the top of query 3
        self.queries = q
        # masks: ~70 % of the rows, group 5 emptied, stray bits beyond `size` set
        keep = rng.random((65, n)) < 0.7
        keep[:, groups == 5] = False
        self.keep_shared, self.keep_each = keep[64], keep[:64]
        self.stride = ((n + 31) // 32) * 4 + 4            # wider than it has to be
        self.mask_shared = self.pack(self.keep_shared[None], ((n + 31) // 32) * 4)[0]
        self.mask_each = self.pack(self.keep_each, self.stride)

    def pack(self, keep, stride):
        out = np.zeros((keep.shape[0], stride * 8), dtype=bool)
        out[:, :self.n] = keep
        out[:, self.n:((self.n + 31) // 32) * 32] = True  # stray bits of the last word
        return np.packbits(out, axis=1, bitorder="little")


def build(data, mirror: bool = True, rows=None, ids=None, extra: int = 8) -> DenseIndex:
    old = os.environ.pop("CRAG_NO_FP16_MIRROR", None)
    try:
        if not mirror:
            os.environ["CRAG_NO_FP16_MIRROR"] = "1"     # read once, at crag_index_create
        ix = DenseIndex(data.dim, capacity=data.n + extra, device=0)
    finally:
        os.environ.pop("CRAG_NO_FP16_MIRROR", None)
        if old is not None:
            os.environ["CRAG_NO_FP16_MIRROR"] = old
    ix.add(data.rows if rows is None else rows, data.ids if ids is None else ids)
    return ix


def lane_scores(ix: DenseIndex, queries, stored_ids) -> np.ndarray:
    """[nq, size] the lane's own score of every (query, stored row): the per-slot scores of the listed-rows search (the
    bits of the masked search), in calls of at most 4096 ids.  NaN: the pair scores nothing."""
    parts = [ix.search_ids(queries, stored_ids[i:i + 4096].tolist(), 1, slot_scores=True)[3]
             for i in range(0, len(stored_ids), 4096)]
    return np.concatenate(parts, axis=1)


def grouped(ix: DenseIndex, queries, k, groups, n_groups, per_group, mask=None, stride=0, want_groups=True, scratch=None):
    """-> ids [nq, k], scores [nq, k], groups [nq, k] (None without), counts [nq] through the async entry, into
    sentinel-filled outputs."""
    nq = int(queries.shape[0])
    out_ids = torch.full((nq, k), -7, dtype=torch.int64, device=DEV)
    out_sc = torch.full((nq, k), -7.0, dtype=torch.float32, device=DEV)
    out_grp = torch.full((nq, k), -7, dtype=torch.int32, device=DEV) if want_groups else None
    out_ct = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    d_mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    ix.search_grouped_async(torch.from_numpy(np.ascontiguousarray(queries)).to(DEV), k,
                            torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(DEV), n_groups, per_group,
                            out_ids, out_sc, out_ct, out_grp, d_row_mask=d_mask, mask_stride=stride, scratch=scratch,
                            stream=torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize(DEV)
    return (out_ids.cpu().numpy(), out_sc.cpu().numpy(), None if out_grp is None else out_grp.cpu().numpy(),
            out_ct.cpu().numpy())


def oracle(scores, ids, groups, n_groups, keep, k, per_group):
    """the walk for every query over the lane's scores; keep: [n] shared, [nq, n] per query or None"""
    res = []
    for q in range(scores.shape[0]):
        ok = ~np.isnan(scores[q])
        if keep is not None:
            ok &= keep if keep.ndim == 1 else keep[q]
        res.append(capped_topk(scores[q], ids, groups, ok, k, per_group, n_groups))
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
            np.asarray([r[3] for r in res], dtype=np.int32))


def assert_same(got, want, note=""):
    assert np.array_equal(got[3], want[3]), (note, got[3], want[3])
    assert np.array_equal(got[0], want[0]), note
    assert np.array_equal(bits(got[1]), bits(want[1])), note
    if got[2] is not None and want[2] is not None:
        assert np.array_equal(got[2], want[2]), note


CASES = {"mirror": (1024, True, 5), "rows-only": (1024, False, 5), "dim-260": (260, True, 31)}


@pytest.fixture(scope="module", params=list(CASES))
def case(gpu, request):
    dim, mirror, seed = CASES[request.param]
    data = Data(N_ROWS, dim, seed)
    ix = build(data, mirror=mirror)
    assert ix.prefilter_row_bytes() == (2048 if mirror else 4096)
    scores = lane_scores(ix, data.queries, data.ids)       # computed once, shared, never changed
    scores.setflags(write=False)
    yield data, ix, scores
    ix.close()


@pytest.fixture(scope="module")
def plain(gpu):
    data = Data(N_ROWS, 1024, 5)
    ix = build(data)
    yield data, ix
    ix.close()


@pytest.mark.parametrize("form", ["no-mask", "shared-mask", "per-query-masks"])
def test_equals_the_oracle(case, form):
    data, ix, scores = case
    assert np.isnan(scores[1]).all() and np.isnan(scores[2]).all()              # the zero and the non-finite query
    assert np.isnan(scores[0, data.zero_pos]) and np.isnan(scores[0, data.nan_pos])
    capped = False
    for nq in NQS:
        mask, stride, keep = {"no-mask": (None, 0, None), "shared-mask": (data.mask_shared, 0, data.keep_shared),
                              "per-query-masks": (data.mask_each[:nq], data.stride, data.keep_each[:nq])}[form]
        for k in KS:
            for per in PERS:
                got = grouped(ix, data.queries[:nq], k, data.groups, N_GROUPS, per, mask, stride)
                want = oracle(scores[:nq], data.ids, data.groups, N_GROUPS, keep, k, per)
                assert_same(got, want, (form, nq, k, per))
                if nq >= 3:
                    assert got[3][1] == 0 and got[3][2] == 0
                assert not np.isin(got[2], [1, N_GROUPS] + ([5] if keep is not None else [])).any()
                capped = capped or (per < 8 and k >= 32 and int(got[3][0]) < k)
    assert capped   # the cap did bind: fewer than k rows although ~ 200 are eligible


def test_layouts_and_batch_sizes_agree_bit_for_bit(gpu):
    """A pair's score depends on the pair alone: not on the row layout, nq, k or per_group."""
    data = Data(N_ROWS, 1024, 5)
    with build(data) as a, build(data, mirror=False) as b:
        whole = grouped(a, data.queries, 128, data.groups, N_GROUPS, 8)
        assert_same(grouped(b, data.queries, 128, data.groups, N_GROUPS, 8), whole)
        one = grouped(a, data.queries[5:6], 128, data.groups, N_GROUPS, 8)
        assert_same(one, tuple(x[5:6] for x in whole))
        score_of = dict(zip(whole[0][5, :whole[3][5]].tolist(), bits(whole[1][5, :whole[3][5]]).tolist()))
        few = grouped(b, data.queries[4:6], 7, data.groups, N_GROUPS, 1)
        assert few[3][1] == 7 and all(score_of[int(i)] == int(s) for i, s in zip(few[0][1], bits(few[1][1])))


def test_equals_the_plain_search_when_the_cap_cannot_bind(plain):
    data, ix = plain
    queries = data.queries[:5]
    small = (np.arange(N_ROWS) * 7 % 40).astype(np.int32)            # 40 groups of 5 rows: per_group = 8 never binds
    own = np.arange(N_ROWS, dtype=np.int32)                          # every row its own group
    packed = DenseIndex.pack_mask(data.keep_shared)
    for k in range(1, _native.CRAG_MAX_K + 1):                       # every k
        want = ix.search(queries, k)
        for groups, n_groups, per in ((small, 40, 8), (own, N_ROWS, 1)):
            got = grouped(ix, queries, k, groups, n_groups, per)
            assert_same(got, (want[0], want[1], None, want[2]), (k, n_groups))
        if k in KS:
            want = ix.search(queries, k, row_mask=packed)
            got = grouped(ix, queries, k, small, 40, 8, mask=packed)
            assert_same(got, (want[0], want[1], None, want[2]), (k, "masked"))


def test_ties_go_to_the_lower_id(plain):
    data, ix = plain
    got = grouped(ix, data.queries[:4], 10, data.groups, N_GROUPS, 1)
    lo, hi = (int(data.ids[p]) for p in data.inside)
    assert got[0][0, 0] == lo and hi not in got[0][0] and got[2][0, 0] == 2       # inside a group: the lower id wins
    two = grouped(ix, data.queries[:4], 10, data.groups, N_GROUPS, 2)
    assert two[0][0, :2].tolist() == [lo, hi] and bits(two[1][0, :1]) == bits(two[1][0, 1:2])
    lo, hi = (int(data.ids[p]) for p in data.across)
    assert got[0][3, :2].tolist() == [lo, hi] and bits(got[1][3, :1]) == bits(got[1][3, 1:2])   # across groups: both
    assert sorted(got[2][3, :2].tolist()) == [3, 4]


class Slope:
    """40 000 rows of dim 64 in 7 groups, one query; row = a * q + noise with the noise orthogonal to q and of one
    length, so the score grows with a.  Against the position the score ascends in group 0 (every row displaces the
    whole cascade), descends in group 1 (after the first rows nothing passes the last slot) and is shuffled elsewhere."""

    def __init__(self) -> None:
        n, dim = 40000, 64
        rng = np.random.default_rng(77)
        q = rng.standard_normal(dim)
        groups = (np.arange(n) % 7).astype(np.int32)
        a = rng.permutation(n) * (1.8 / n) + 0.2
        for grp, sign in ((0, 1), (1, -1)):
            where = np.flatnonzero(groups == grp)
            a[where] = np.sort(a[where])[::sign]
        noise = rng.standard_normal((n, dim))
        noise -= np.outer(noise @ q / (q @ q), q)
        noise *= np.linalg.norm(q) / np.linalg.norm(noise, axis=1, keepdims=True)
        self.rows = (np.outer(a, q) + noise).astype(np.float32)
        self.queries = q.astype(np.float32)[None]
        self.n, self.dim, self.groups = n, dim, groups
        self.ids = 10 + 3 * np.arange(n, dtype=np.int64)


@pytest.fixture(scope="module")
def slope(gpu):
    data = Slope()
    ix = build(data)
    scores = lane_scores(ix, data.queries, data.ids)
    assert (np.diff(scores[0, data.groups == 0]) > 0).all() and (np.diff(scores[0, data.groups == 1]) < 0).all()
    want = oracle(scores, data.ids, data.groups, 7, None, 21, 3)
    yield data, ix, want
    ix.close()


def test_the_cascade_in_every_arrival_order(slope):
    data, ix, want = slope
    assert want[3][0] == 21 and np.bincount(want[2][0]).tolist() == [3] * 7
    assert_same(grouped(ix, data.queries, 21, data.groups, 7, 3), want)
    assert_same(grouped(ix, data.queries, 5, data.groups, 7, 3), tuple(x[:, :5] if x.ndim == 2 else np.minimum(x, 5) for x in want))


def test_same_bits_every_time_on_a_dirty_scratch(slope):
    data, ix, want = slope
    scratch = torch.full((DenseIndex.search_grouped_scratch_bytes(1, 7, 3),), 0xFF, dtype=torch.uint8, device=DEV)
    for _ in range(3):
        scratch.fill_(0xFF)
        assert_same(grouped(ix, data.queries, 21, data.groups, 7, 3, scratch=scratch), want)


def test_a_table_of_slots_beyond_one_buffer(gpu):
    """5 000 groups x 2 slots = 10 000 slots per query: the select kernel's buffer holds 4 096 keys."""
    n, dim = 5000, 64
    rng = np.random.default_rng(3)
    data = type("D", (), dict(rows=rng.standard_normal((n, dim)).astype(np.float32), n=n, dim=dim,
                              ids=10 + 3 * np.arange(n, dtype=np.int64)))
    queries = rng.standard_normal((3, dim)).astype(np.float32)
    own = np.arange(n, dtype=np.int32)
    with build(data) as ix:
        scores = lane_scores(ix, queries, data.ids)
        got = grouped(ix, queries, 128, own, n, 2)
        assert_same(got, oracle(scores, data.ids, own, n, None, 128, 2))
        assert got[3].tolist() == [128] * 3
        want = ix.search(queries, 128)
        assert_same(got, (want[0], want[1], None, want[2]))
        keep = np.zeros((3, n), dtype=bool)                          # counts below k: 50, 0 and 4 097 eligible rows
        keep[0, rng.choice(n, size=50, replace=False)] = True
        keep[2, rng.choice(n, size=4097, replace=False)] = True
        stride = ((n + 31) // 32) * 4
        packed = np.packbits(np.pad(keep, ((0, 0), (0, stride * 8 - n))), axis=1, bitorder="little")
        got = grouped(ix, queries, 128, own, n, 2, mask=packed, stride=stride)
        assert_same(got, oracle(scores, data.ids, own, n, keep, 128, 2))
        assert got[3].tolist() == [50, 0, 128]
        pairs = (np.arange(n) // 2).astype(np.int32)                 # 2 500 groups of two neighbours, one slot each
        assert_same(grouped(ix, queries, 128, pairs, 2500, 1), oracle(scores, data.ids, pairs, 2500, None, 128, 1))


def test_after_remove_and_insert(gpu):
    data = Data(N_ROWS, 1024, 5)
    late = np.asarray([30, 31, 95, 150])
    gone = np.asarray([3, 40, 41, 97, 160])
    start = np.setdiff1d(np.arange(N_ROWS), late)
    final = np.setdiff1d(np.arange(N_ROWS), gone)
    queries = data.queries[:6]
    with build(data, rows=data.rows[start], ids=data.ids[start]) as ix, \
            build(data, rows=data.rows[final], ids=data.ids[final]) as fresh:
        ix.remove(data.ids[gone])
        ix.insert(data.rows[late], data.ids[late])                   # rows between stored ids
        assert len(ix) == len(fresh) == len(final)
        groups = data.groups[final]                                  # the group column, rebuilt for the new positions
        for k, per in ((50, 2), (128, 8), (10, 1)):
            got = grouped(ix, queries, k, groups, N_GROUPS, per)
            assert_same(got, grouped(fresh, queries, k, groups, N_GROUPS, per), (k, per))
            assert not np.isin(got[0], data.ids[gone]).any()
        scores = lane_scores(fresh, queries, data.ids[final])
        assert_same(grouped(ix, queries, 50, groups, N_GROUPS, 2), oracle(scores, data.ids[final], groups, N_GROUPS, None, 50, 2))


def test_without_the_groups_output(plain):
    data, ix = plain
    full = grouped(ix, data.queries[:6], 33, data.groups, N_GROUPS, 2)
    bare = grouped(ix, data.queries[:6], 33, data.groups, N_GROUPS, 2, want_groups=False)
    assert bare[2] is None
    assert_same(bare, full)


def test_host_form_an_empty_index_and_argument_errors(gpu, plain):
    data, ix = plain
    want = grouped(ix, data.queries[:6], 33, data.groups, N_GROUPS, 2, data.mask_each[:6], data.stride)
    host = ix.search_grouped(data.queries[:6], 33, data.groups, N_GROUPS, 2, row_mask=data.mask_each[:6])
    assert_same(host, want)
    dev = ix.search_grouped(torch.from_numpy(data.queries[:6]).to(DEV), 33, torch.from_numpy(data.groups).to(DEV), N_GROUPS,
                            2, row_mask=torch.from_numpy(data.mask_each[:6]).to(DEV))
    assert_same(dev, want)
    for bad in (dict(k=0), dict(k=129), dict(per_group=0), dict(per_group=9), dict(n_groups=0)):
        args = dict(k=5, n_groups=N_GROUPS, per_group=2)
        args.update(bad)
        with pytest.raises(ValueError):
            ix.search_grouped(data.queries[:2], args["k"], data.groups, args["n_groups"], args["per_group"])
    # the split that keeps the scratch at or below the limit changes nothing
    old = DenseIndex.GROUPED_SCRATCH_LIMIT
    try:
        DenseIndex.GROUPED_SCRATCH_LIMIT = 3 * DenseIndex.search_grouped_scratch_bytes(1, N_GROUPS, 2)
        assert_same(ix.search_grouped(data.queries[:6], 33, data.groups, N_GROUPS, 2, row_mask=data.mask_each[:6]), want)
    finally:
        DenseIndex.GROUPED_SCRATCH_LIMIT = old
    # a stride below ceil(size / 32) * 4 is refused like crag_index_search refuses it, and nothing is enqueued
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    d_q = torch.from_numpy(data.queries[:2].copy()).to(DEV)
    d_grp = torch.from_numpy(data.groups).to(DEV)
    d_mask = torch.from_numpy(data.mask_each[:2].copy()).to(DEV)
    outs = [torch.full((2, 5), -7, dtype=torch.int64, device=DEV), torch.full((2, 5), -7.0, dtype=torch.float32, device=DEV),
            torch.full((2,), -7, dtype=torch.int32, device=DEV)]
    scratch = torch.empty(DenseIndex.search_grouped_scratch_bytes(2, N_GROUPS, 2), dtype=torch.uint8, device=DEV)

    def call(stride):
        return gpu.crag_index_search_grouped_async(ix._h, d_q.data_ptr(), 2, 5, d_grp.data_ptr(), N_GROUPS, 2, d_mask.data_ptr(),
                                                   stride, outs[0].data_ptr(), outs[1].data_ptr(), None, outs[2].data_ptr(),
                                                   scratch.data_ptr(), int(scratch.numel()), st)

    assert call(24) == -1 and b"search_grouped" in gpu.crag_last_error()      # 200 rows need 28 bytes
    torch.cuda.synchronize(DEV)
    assert bool((outs[0] == -7).all()) and bool((outs[2] == -7).all())
    assert call(data.stride) == 0
    torch.cuda.synchronize(DEV)
    assert outs[2].tolist() == [int(want[3][0]) if want[3][0] < 5 else 5, 0]
    with DenseIndex(1024, capacity=64, device=0) as empty:                    # an empty index: every count is 0
        got = grouped(empty, np.ones((2, 1024), dtype=np.float32), 5, np.zeros(1, dtype=np.int32), 3, 2)
        assert got[3].tolist() == [0, 0] and (got[0] == -1).all() and np.isnan(got[1]).all() and (got[2] == -1).all()
        host = empty.search_grouped(np.ones((2, 1024), dtype=np.float32), 5, np.zeros(0, dtype=np.int32), 3, 2)
        assert host[3].tolist() == [0, 0] and (host[0] == -1).all()


def make_tables():
    """300 chunks of 20 calls; call 0 is a long call: its 60 chunks are the 60 best rows of the query."""
    from datetime import datetime, timedelta
    from uuid import UUID
    n, t0 = 300, datetime(2026, 3, 1)
    rng = np.random.default_rng(9)
    q = rng.standard_normal(1024).astype(np.float32)
    rows = rng.standard_normal((n, 1024)).astype(np.float32)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(20)]
    call_of = np.asarray([0 if i % 5 == 0 else 1 + (i * 7) % 19 for i in range(n)])
    long_rows = np.flatnonzero(call_of == 0)
    rows[long_rows] += np.outer(rng.uniform(1.0, 3.0, size=long_rows.size), q).astype(np.float32)
    cols = {"chunk_id": [1000 + 2 * i for i in range(n)], "call_id": [calls[c]["call_id"] for c in call_of],
            "text": [f"row {i}" for i in range(n)], "speaker": ["S%d" % (i % 3) for i in range(n)],
            "start_ts_ms": [i * 10 for i in range(n)], "end_ts_ms": [i * 10 + 9 for i in range(n)]}
    chunks = rt.DenseTable("chunks", "chunk_id", dim=1024, capacity=n + 64)
    arts = rt.DenseTable("artifact_chunks", "artifact_chunk_id", dim=1024, capacity=64)
    chunks.add(rows, cols, call_started_at=[t0 + timedelta(days=i % 6) for i in range(n)],
               call_tags={c["call_id"]: ["billing"] if i % 2 else ["outage"] for i, c in enumerate(calls)})
    arts.add(rows[:30], {"artifact_chunk_id": list(range(500, 530)), "call_id": [calls[0]["call_id"]] * 30,
                         "artifact_id": [i // 3 for i in range(30)], "kind": ["summary"] * 30,
                         "content": [f"artifact {i}" for i in range(30)]},
             call_started_at=[t0] * 30)
    return chunks, arts, calls, q, call_of, t0


def table_oracle(chunks, q, call_of, keep, k, per):
    ids = np.asarray(chunks.columns["chunk_id"], dtype=np.int64)
    scores = lane_scores(chunks.index, q[None], ids)
    ok = ~np.isnan(scores[0]) if keep is None else (~np.isnan(scores[0]) & keep)
    return capped_topk(scores[0], ids, call_of, ok, k, per, int(call_of.max()) + 1)


def test_through_the_table(gpu):
    from datetime import timedelta
    chunks, arts, calls, q, call_of, t0 = make_tables()
    try:
        F = rt.RetrieveFilters
        ids5 = [c["call_id"] for c in calls[:5]]
        plain_rows = chunks.fetch_dense(q, None, None, "ann", 50, rt.CHUNK_SELECT)
        assert sum(r["call_id"] == calls[0]["call_id"] for r in plain_rows) == 50    # the long call fills the lane
        for filters, call_ids in ((None, None), (F(date_from=t0 + timedelta(days=2)), None), (F(), ids5),
                                  (F(call_tags=["outage"]), None), (F(), [])):
            keep = chunks.filter_mask(filters, call_ids)
            want = table_oracle(chunks, q, call_of, keep, 50, 2)
            rows = chunks.fetch_dense(q, filters, call_ids, "ann", 50, rt.CHUNK_SELECT, per_call=2)
            assert [r["chunk_id"] for r in rows] == want[0][:want[3]].tolist(), (filters, call_ids)
            assert np.array_equal(bits([r["score"] for r in rows]), bits(want[1][:want[3]]))
            assert all(set(r) == set(rt.CHUNK_SELECT) | {"score"} for r in rows)
            per_call = {}
            for r in rows:
                per_call[r["call_id"]] = per_call.get(r["call_id"], 0) + 1
            assert not rows or max(per_call.values()) <= 2
            best = table_oracle(chunks, q, call_of, keep, 7, 1)
            short = chunks.shortlist_calls(q, filters, call_ids, 7)
            assert [(c, i) for c, i, _ in short] == [(calls[g]["call_id"], int(i)) for g, i in zip(best[2][:best[3]], best[0][:best[3]])]
            assert np.array_equal(bits([s for _, _, s in short]), bits(best[1][:best[3]]))
        assert len(chunks.fetch_dense(q, None, None, "ann", 50, rt.CHUNK_SELECT, per_call=2)) == 40   # 20 calls x 2
        assert chunks.shortlist_calls(q, None, None, 3)[0][0] == calls[0]["call_id"]
        # a call-scoped request small enough for the listed-rows route still holds the cap
        assert settings.embeddings_exact_scan_threshold >= 60
        rows = chunks.fetch_dense(q, F(), ids5[:1], "exact", 50, rt.CHUNK_SELECT, per_call=2)
        assert len(rows) == 2
    finally:
        chunks.close(); arts.close()


def test_the_backend_and_the_knob(gpu, monkeypatch):
    from cadence_rag_amd import embeddings
    chunks, arts, calls, q, call_of, t0 = make_tables()
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[q.tolist() for _ in texts], model="m"))
    monkeypatch.setattr(settings, "evidence_dedupe_cosine", 0.0)
    monkeypatch.setattr(settings, "rerank_base_url", "")

    class Before(rt.GpuRetrieveBackend):
        """the chunk dense lane as it was before the knob existed"""
        def fetch_chunks_dense(self, query_embedding, filters, call_ids, mode, limit):
            return rt._fetch_chunks_dense(self.tables["chunks"], query_embedding, filters, call_ids, mode, limit)

    def response(backend, **kw):
        out = rt.retrieve_evidence(rt.RetrieveRequest(query="why did the renewal slip", debug=True, **kw), backend=backend)
        out.pop("query_id")
        return out

    try:
        be = rt.GpuRetrieveBackend(chunks, arts, calls=calls)
        monkeypatch.setattr(settings, "dense_per_call_cap", 0)
        off = response(be)
        assert off == response(Before(chunks, arts, calls=calls))
        assert "dense_per_call_cap" not in off["notes"]["retrieval"]
        lane = off["debug"]["lanes"]["chunks"]["dense"]
        long_ids = set(np.asarray(chunks.columns["chunk_id"])[call_of == 0].tolist())
        assert len(lane) == 50 and all(r["chunk_id"] in long_ids for r in lane)   # uncapped: 50 rows of one call
        assert len({item["call_id"] for item in off["quotes"]}) == 1

        monkeypatch.setattr(settings, "dense_per_call_cap", 2)
        on = response(be)
        assert on["notes"]["retrieval"]["dense_per_call_cap"] == 2
        want = table_oracle(chunks, q, call_of, None, 50, 2)
        lane = on["debug"]["lanes"]["chunks"]["dense"]
        assert [r["chunk_id"] for r in lane] == want[0][:want[3]].tolist() and len(lane) == 40
        assert np.array_equal(bits([r["score"] for r in lane]), bits(want[1][:want[3]]))
        assert sum(r["chunk_id"] in long_ids for r in lane) == 2
        assert len({item["call_id"] for item in on["quotes"]}) > 1                # the pack now reaches other calls
        assert on["debug"]["lanes"]["artifacts"] == off["debug"]["lanes"]["artifacts"]   # that side stays uncapped
        assert len(on["debug"]["lanes"]["artifacts"]["dense"]) > 2
        rows = be.fetch_chunks_dense(q, None, None, "ann", 50)
        assert [r["chunk_id"] for r in rows] == want[0][:want[3]].tolist()
        monkeypatch.setattr(settings, "dense_per_call_cap", 50)                  # clamped to CRAG_GROUP_MAX_PER
        rows = be.fetch_chunks_dense(q, None, None, "ann", 50)
        assert sum(r["chunk_id"] in long_ids for r in rows) == _native.CRAG_GROUP_MAX_PER
        assert response(be)["notes"]["retrieval"]["dense_per_call_cap"] == _native.CRAG_GROUP_MAX_PER
    finally:
        chunks.close(); arts.close()
