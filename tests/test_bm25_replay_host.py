"""tests/bm25_replay.py (the fp32 reference of the exact GPU tests) held to tests/bm25_oracle.py (fp64) on the Zipf
corpus and the 64 queries of test_bm25_gpu.py, without a device: every score within bm25_oracle.tolerance(T) of the
oracle's, every id that differs from the oracle's order inside that window -- the rule of assert_matches."""
import numpy as np
import pytest

from bm25_oracle import Bm25Oracle, assert_matches
from bm25_replay import NAN_BITS, replay, replay_index
from cadence_rag_amd.bm25 import Bm25Index
from test_bm25_gpu import zipf_corpus


@pytest.fixture(scope="module")
def zipf_host():
    rng, texts, words, p = zipf_corpus(2024, 20000, 5000, 5, 120)          # the `zipf` fixture of test_bm25_gpu.py
    ids = np.arange(20000, dtype=np.int64) * 3 + 100
    queries = [" ".join(rng.choice(words, size=int(rng.integers(1, 33)), p=p)) for _ in range(64)]
    index = Bm25Index(texts, ids, "cpu")                                   # host arrays only: nothing is launched
    return index, Bm25Oracle(texts, ids), queries


@pytest.mark.parametrize("k", [1, 50, 128])
def test_replay_against_the_fp64_oracle(zipf_host, k):
    index, oracle, queries = zipf_host
    rng = np.random.default_rng(9)
    worst = 0.0
    for eligible in (None, rng.random(20000) < 0.3):
        ids, bits, ct = replay_index(index, *index.query_terms(queries), k, eligible)
        for q, text in enumerate(queries):
            worst = max(worst, assert_matches(oracle, text, k, ids[q], bits[q].view(np.float32), ct[q], eligible))
    print(f"k={k}: replay's worst score error = {worst:.4f} of the single bound (T + 9) * 2^-24")


def test_replay_order_padding_and_masks():
    """Hand-checkable: three rows, two terms, avgdl 2.  Row 0 and row 2 are twins (equal bits, lower position first)."""
    post_ptr = np.array([0, 3, 4], dtype=np.int64)
    post_pos = np.array([0, 1, 2, 1], dtype=np.int32)
    post_tf = np.array([1, 5, 1, 1], dtype=np.uint16)
    doc_len = np.array([1, 3, 1], dtype=np.int32)
    ids = np.array([10, 20, 30], dtype=np.int64)
    args = (post_ptr, post_pos, post_tf, doc_len, 2.0)
    one = np.float32(1.0) / (np.float32(1.0) + (np.float32(0.5) * np.float32(0.75) + np.float32(0.25)) * np.float32(1.2))
    got_ids, got_bits, n = replay(*args, [0], np.array([2.0], np.float32), 4, ids)
    assert n == 3 and got_ids.tolist() == [20, 10, 30, -1] and got_bits[3] == NAN_BITS
    assert got_bits[1] == got_bits[2] == (np.float32(2.0) * one).view(np.uint32)
    got_ids, _, n = replay(*args, [0], np.array([2.0], np.float32), 2, None, eligible=np.array([False, True, True]))
    assert n == 2 and got_ids.tolist() == [1, 2]
    got_ids, got_bits, n = replay(*args, [1], np.array([1.0], np.float32), 2, ids)
    assert n == 1 and got_ids.tolist() == [20, -1]
    # terms are summed in ascending id whatever the order they are handed in
    a = replay(*args, [0, 1], np.array([0.1, 0.7], np.float32), 3, ids)
    b = replay(*args, [1, 0], np.array([0.7, 0.1], np.float32), 3, ids)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert replay(*args, [], np.empty(0, np.float32), 2, ids)[2] == 0
