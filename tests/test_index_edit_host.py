"""Host half of the in-place index edits: the numpy oracle against hand-written cases, and the three ABI entries in
the header and in the ctypes table with one signature."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from cadence_rag_amd import _native
from tests import index_edit_oracle as ox

HEADER = (Path(__file__).resolve().parent.parent / "include" / "crag_dense.h").read_text()
IDS = np.array([10, 20, 30, 40, 50], dtype=np.int64)
ROWS = np.arange(5 * 4, dtype=np.float32).reshape(5, 4)


def test_oracle_remove_by_hand():
    ids, rows, removed = ox.remove(IDS, ROWS, [40, 7, 10, 40, 99])
    assert ids.tolist() == [20, 30, 50] and removed == 2
    assert np.array_equal(rows, ROWS[[1, 2, 4]])
    ids, rows, removed = ox.remove(IDS, ROWS, [1, 2, 3])
    assert ids.tolist() == IDS.tolist() and removed == 0 and np.array_equal(rows, ROWS)
    ids, rows, removed = ox.remove(IDS, ROWS, IDS[::-1])
    assert ids.size == 0 and rows.shape == (0, 4) and removed == 5


def test_oracle_compact_by_hand():
    ids, rows = ox.compact(IDS, ROWS, [True, False, False, True, True])
    assert ids.tolist() == [10, 40, 50] and np.array_equal(rows, ROWS[[0, 3, 4]])
    with pytest.raises(ValueError):
        ox.compact(IDS, ROWS, [True, False])
    assert ox.pack_keep([True, False, False, True, True]).tolist() == [0b11001, 0, 0, 0]
    assert ox.pack_keep([True] * 33).tolist() == [255, 255, 255, 255, 1, 0, 0, 0]


def test_oracle_insert_by_hand():
    new = np.array([[100, 101, 102, 103], [200, 201, 202, 203], [300, 301, 302, 303]], dtype=np.float32)
    ids, rows = ox.insert(IDS, ROWS, [5, 35, 60], new)
    assert ids.tolist() == [5, 10, 20, 30, 35, 40, 50, 60]
    assert np.array_equal(rows, np.stack([new[0], ROWS[0], ROWS[1], ROWS[2], new[1], ROWS[3], ROWS[4], new[2]]))
    with pytest.raises(ValueError, match="stored already"):
        ox.insert(IDS, ROWS, [5, 30], new[:2])
    with pytest.raises(ValueError, match="ascend"):
        ox.insert(IDS, ROWS, [35, 5], new[:2])
    ids, rows = ox.insert(np.empty(0, np.int64), np.empty((0, 4), np.float32), [3, 4], new[:2])
    assert ids.tolist() == [3, 4] and np.array_equal(rows, new[:2])


def test_oracle_edits_compose_to_a_fresh_build():
    """remove then insert of the same rows gives the table back: the oracle's own statement of the contract."""
    ids, rows, _ = ox.remove(IDS, ROWS, [20, 40])
    ids, rows = ox.insert(ids, rows, [20, 40], ROWS[[1, 3]])
    assert np.array_equal(ids, IDS) and np.array_equal(rows, ROWS)


def test_oracle_update_by_hand():
    new = np.array([[100, 101, 102, 103], [200, 201, 202, 203]], dtype=np.float32)
    ids_before, rows_before, new_before = IDS.copy(), ROWS.copy(), new.copy()
    ids, rows = ox.update(IDS, ROWS, 3, new)
    assert np.array_equal(IDS, ids_before) and np.array_equal(ROWS, rows_before) and np.array_equal(new, new_before)
    assert ids is not IDS and rows is not ROWS and not np.shares_memory(rows, ROWS) and not np.shares_memory(rows, new)
    assert np.array_equal(ids, IDS)
    assert np.array_equal(rows, np.stack([ROWS[0], ROWS[1], ROWS[2], new[0], new[1]]))
    ids, rows = ox.update(IDS, ROWS, 0, new[1])                     # one row given as a vector
    assert np.array_equal(ids, IDS) and np.array_equal(rows, np.stack([new[1], ROWS[1], ROWS[2], ROWS[3], ROWS[4]]))
    ids, rows = ox.update(IDS, ROWS, 5, np.empty((0, 4), np.float32))   # n == 0 is allowed anywhere up to the size
    assert np.array_equal(ids, IDS) and np.array_equal(rows, ROWS)
    for pos in (-1, 4, 5):
        with pytest.raises(ValueError, match="outside"):
            ox.update(IDS, ROWS, pos, new)
    with pytest.raises(ValueError, match="width"):
        ox.update(IDS, ROWS, 0, new[:, :3])


_C_TYPES = {"crag_index *": ctypes.c_void_p, "const int64_t *": ctypes.c_void_p, "const float *": ctypes.c_void_p,
            "const uint8_t *": ctypes.c_void_p, "int64_t *": ctypes.POINTER(ctypes.c_int64), "int64_t": ctypes.c_int64}


@pytest.mark.parametrize("name", ["crag_index_remove", "crag_index_compact", "crag_index_insert"])
def test_header_and_binding_declare_one_signature(name):
    m = re.search(r"^int " + name + r"\(([^)]*)\);", HEADER, re.M)
    assert m, f"{name} is not declared in include/crag_dense.h"
    want = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\w+$", "", arg.strip()).strip()     # drop the parameter name
        want.append(_C_TYPES[ctype])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert argtypes == want


def test_header_says_what_the_edits_replace_and_wait_for():
    text = " ".join(HEADER.split())
    for name in ("crag_index_remove", "crag_index_compact", "crag_index_insert", "CRAG_EDIT_CHUNK_ROWS"):
        assert name in text
    assert "ON DELETE CASCADE" in text and "0001_initial_schema.py:59,79,123" in text
    assert "0006_add_artifact_chunks.py:23-24" in text
    assert "app/embedding_pipeline.py" in text and "arbitrary id order" in text
    assert "WAIT FOR EVERY SEARCH IN FLIGHT" in text and "pipe streams" in text
