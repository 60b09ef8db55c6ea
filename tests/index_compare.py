"""What "indistinguishable from a second index built fresh" means in the GPU tests of the index:
size, ids, get_rows bits, every search's ids / score bits / counts, the scan kernel chosen and count_eligible, with and
without a row mask.  Shared by tests/test_index_edit_gpu.py (remove / compact / insert) and
tests/test_index_store_gpu.py (add in pieces / update).  Every comparison is an equality."""
import numpy as np

from cadence_rag_amd.dense_index import DenseIndex

MODES = {"mirror": {}, "no_mirror": {"CRAG_NO_FP16_MIRROR": "1"}, "no_prefilter": {"CRAG_NO_PREFILTER": "1"}}


def _env(monkeypatch, mode="mirror", chunk="64"):
    """The switches are read once, when an index is created."""
    for key in ("CRAG_NO_FP16_MIRROR", "CRAG_NO_PREFILTER", "CRAG_EDIT_CHUNK_ROWS"):
        monkeypatch.delenv(key, raising=False)
    for key, val in MODES[mode].items():
        monkeypatch.setenv(key, val)
    if chunk is not None:
        monkeypatch.setenv("CRAG_EDIT_CHUNK_ROWS", chunk)


def _build(rows, ids, capacity=None):
    ix = DenseIndex(rows.shape[1], capacity=capacity or max(len(ids), 1))
    if len(ids):
        ix.add(rows, ids=ids)
    return ix


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_same(edited, fresh, queries, ks=(10,), seed=0, stats=False):
    """`edited` is indistinguishable from `fresh`; returns nothing, asserts equalities only."""
    n = len(fresh)
    assert len(edited) == n
    if n:
        r1, i1 = edited.get_rows(0, n)
        r2, i2 = fresh.get_rows(0, n)
        assert np.array_equal(i1, i2)
        assert np.array_equal(_bits(r1), _bits(r2))
    mask = DenseIndex.pack_mask(np.random.default_rng(seed).random(max(n, 1)) < 0.5)[: ((n + 31) // 32) * 4]
    for m in (None, mask):
        assert edited.count_eligible(m) == fresh.count_eligible(m)
        if n == 0:
            continue
        for k in ks:
            if stats:
                edited.prefilter_stats(), fresh.prefilter_stats()     # reading clears them
            a = edited.search(queries, k, row_mask=m)
            b = fresh.search(queries, k, row_mask=m)
            assert np.array_equal(a[0], b[0])
            assert np.array_equal(_bits(a[1]), _bits(b[1]))
            assert np.array_equal(a[2], b[2])
            assert edited.last_scan_kernel() == fresh.last_scan_kernel()
            if stats:
                assert edited.prefilter_stats()["rescored_rows"] == fresh.prefilter_stats()["rescored_rows"]
