"""The references of tests/test_fusion_gpu.py checked against independent statements of the same contracts: the host
mirror of the reference's _rrf_merge, helpers.cpu_merge_topk and a naive set-intersection loop.  CPU only."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

import fusion_oracle as fo
from helpers import cpu_merge_topk

from cadence_rag_amd import retrieve as rt

GOLD = json.loads((Path(__file__).parent / "golden" / "reference_host_logic.json").read_text())


def _rrf_via_host_mirror(lists, rrf_k):
    """One query through retrieve._rrf_merge: (ids, scores, masks) in its order."""
    names = [f"lane{l}" for l in range(len(lists))]
    merged = rt._rrf_merge({nm: [{"id": int(v)} for v in ids] for nm, ids in zip(names, lists)}, "id", k=rrf_k)
    return ([m[0]["id"] for m in merged], [m[2] for m in merged],
            [sum(1 << names.index(nm) for nm in m[1]) for m in merged])


def _check_rrf(lists, rrf_k, out_k):
    widths = [max(len(ids), 1) for ids in lists]
    lanes = [np.array([list(ids) + [-5] * (w - len(ids))], dtype=np.int64) for ids, w in zip(lists, widths)]
    counts = [np.array([len(ids)], dtype=np.int32) for ids in lists]
    ids, scores, masks, cnt = fo.rrf(lanes, counts, widths, rrf_k, out_k)
    w_ids, w_sc, w_mask = _rrf_via_host_mirror(lists, rrf_k)
    c = min(len(w_ids), out_k)
    assert int(cnt[0]) == c
    assert ids[0, :c].tolist() == w_ids[:c] and np.all(ids[0, c:] == -1)
    assert scores[0, :c].tolist() == w_sc[:c] and np.all(np.isnan(scores[0, c:]))      # the same floats, bit for bit
    assert masks[0, :c].tolist() == w_mask[:c] and np.all(masks[0, c:] == 0)


def test_rrf_equals_the_host_mirror_on_the_reference_goldens():
    assert GOLD["rrf_merge"]
    for case in GOLD["rrf_merge"]:
        lists = [ids for _, ids in case["lanes"]]
        unique = len({i for ids in lists for i in ids})
        for out_k in (1, max(unique - 1, 1), unique, unique + 1, 1024):
            _check_rrf(lists, 60, out_k)
        ids, scores, _, _ = fo.rrf([np.array([l or [0]], dtype=np.int64) for l in lists],
                                   [np.array([len(l)]) for l in lists], [max(len(l), 1) for l in lists], 60, unique)
        assert ids[0].tolist() == case["order"] and scores[0].tolist() == case["scores"]


def test_rrf_equals_the_host_mirror_with_repeats_inside_a_lane():
    rng = np.random.default_rng(101)
    for case in range(60):
        n_lanes = int(rng.integers(1, 9))
        lists = [rng.integers(0, 12, size=int(rng.integers(0, 30))).tolist() for _ in range(n_lanes)]   # many repeats
        unique = len({i for ids in lists for i in ids})
        for out_k in {1, max(unique - 1, 1), max(unique, 1), unique + 1}:
            _check_rrf(lists, int(rng.choice([0, 1, 60])), out_k)


def test_rrf_clamps_counts_to_the_lane_width():
    lane = np.array([[7, 8, 9]], dtype=np.int64)
    for given, used in ((-4, 0), (0, 0), (2, 2), (3, 3), (9, 3)):
        ids, _, _, cnt = fo.rrf([lane], [np.array([given])], [3], 60, 5)
        assert int(cnt[0]) == used and ids[0, :used].tolist() == [7, 8, 9][:used]


def test_merge_equals_cpu_merge_topk_without_signed_zeros():
    import torch
    rng = np.random.default_rng(102)
    for n_lists, nq, k in ((1, 3, 1), (2, 5, 7), (8, 13, 10), (5, 2, 128)):
        sc = rng.choice(np.array([-2.5, -1.0, 0.25, 0.5, 0.75, 1.0], dtype=np.float32), size=(n_lists, nq, k))
        sc = -np.sort(-sc, axis=2)                                     # lists arrive sorted, ties abound
        ids = rng.integers(0, 50, size=(n_lists, nq, k)).astype(np.int64)
        ct = rng.integers(0, k + 1, size=(n_lists, nq)).astype(np.int32)
        got = fo.merge(ids, sc, ct, k)
        want = cpu_merge_topk(torch.from_numpy(ids), torch.from_numpy(sc), torch.from_numpy(ct))
        assert np.array_equal(got[0], want[0].numpy())
        assert np.array_equal(got[1].view(np.uint32), want[1].numpy().view(np.uint32))
        assert np.array_equal(got[2], want[2].numpy())


def test_merge_ranks_minus_zero_below_plus_zero():
    ids = np.array([[[5, 9]], [[1, 2]]], dtype=np.int64)
    sc = np.array([[[0.0, -1.0]], [[-0.0, -0.0]]], dtype=np.float32)
    got_ids, got_sc, got_ct = fo.merge(ids, sc, np.array([[2], [2]]), 2)
    assert got_ids[0].tolist() == [5, 1] and int(got_ct[0]) == 2          # cpu_merge_topk would answer [1, 2]
    assert got_sc.view(np.uint32)[0].tolist() == [0x00000000, 0x80000000]


def test_tech_lane_equals_a_set_intersection_loop_over_token_strings():
    from cadence_rag_amd.dense_index import DenseIndex
    from cadence_rag_amd.fusion import token_hash
    rng = np.random.default_rng(103)
    n, nq, k = 300, 6, 17
    vocab = [f"TOK-{i}" for i in range(40)]
    row_tokens = [list(rng.choice(vocab, size=int(rng.integers(0, 4)), replace=False)) for _ in range(n)]
    ext = rng.permutation(n).astype(np.int64) * 3 + 1
    order = rng.permutation(n).astype(np.int32)
    queries = [list(rng.choice(vocab, size=int(m), replace=False)) for m in (0, 1, 2, 5, 32, 3)]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(row_tokens[p]) for p in order], out=row_ptr[1:])
    toks = np.array([token_hash(t) for p in order for t in row_tokens[p]], dtype=np.uint64)
    qtok = np.zeros((nq, 32), dtype=np.uint64)
    for q, lst in enumerate(queries):
        qtok[q, :len(lst)] = [token_hash(t) for t in lst]
    qn = np.array([len(lst) for lst in queries], dtype=np.int32)
    elig = rng.random((nq, n)) < 0.5
    for use_mask, stride_extra in ((None, 0), ("shared", 0), ("per", 0), ("per", 8)):
        if use_mask is None:
            mask, stride, ok = None, 0, lambda q, p: True
        elif use_mask == "shared":
            mask, stride, ok = DenseIndex.pack_mask(elig[0]), 0, lambda q, p: elig[0, p]
        else:
            packed = DenseIndex.pack_mask(elig)
            mask = np.zeros((nq, packed.shape[1] + stride_extra), dtype=np.uint8)
            mask[:, :packed.shape[1]] = packed
            stride, ok = mask.shape[1], lambda q, p: elig[q, p]
        got_ids, got_ct = fo.tech_lane(order, row_ptr, toks, ext, qtok, qn, k, mask, stride)
        for q, lst in enumerate(queries):
            want = [int(ext[p]) for p in order if set(row_tokens[p]) & set(lst) and ok(q, p)][:k]
            assert int(got_ct[q]) == len(want) and got_ids[q, :len(want)].tolist() == want
            assert np.all(got_ids[q, len(want):] == -1)
    pos_ids, pos_ct = fo.tech_lane(order, row_ptr, toks, None, qtok, qn, k)
    for q, lst in enumerate(queries):
        assert pos_ids[q, :int(pos_ct[q])].tolist() == [int(p) for p in order if set(row_tokens[p]) & set(lst)][:k]


def test_tech_lane_folds_hash_zero_onto_one():
    order = np.arange(4, dtype=np.int32)
    row_ptr = np.array([0, 1, 2, 3, 3], dtype=np.int64)
    toks = np.array([0, 1, 2], dtype=np.uint64)
    qtok = np.zeros((3, 32), dtype=np.uint64)
    qtok[1, 0], qtok[2, 0] = 1, 2
    ids, ct = fo.tech_lane(order, row_ptr, toks, None, qtok, np.array([1, 1, 1]), 4)
    assert ids[:, :2].tolist() == [[0, 1], [0, 1], [2, -1]] and ct.tolist() == [2, 2, 1]


def test_colliding_fuse_ids_land_in_the_requested_slot():
    for slot, n in ((2047, 1024), (0, 10), (1234, 300)):
        ids = fo.colliding_fuse_ids(slot, n)
        assert ids.dtype == np.int64 and ids.shape == (n,) and np.all(ids >= 0) and np.unique(ids).size == n
        assert all((((int(v) * 0x9E3779B97F4A7C15) % 2 ** 64) >> 40) & 2047 == slot for v in ids)


def test_colliding_tech_hashes_land_in_the_requested_slot():
    for slot, n in ((4095, 2048), (0, 10), (77, 300)):
        hs = fo.colliding_tech_hashes(slot, n)
        assert hs.dtype == np.uint64 and hs.shape == (n,) and np.unique(hs).size == n
        assert all(((int(v) * 0x9E3779B97F4A7C15) % 2 ** 64) >> 52 == slot for v in hs)
