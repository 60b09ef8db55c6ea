"""The contract of the in-place index edits (include/crag_dense.h: crag_index_remove / compact / insert / update) in numpy:
given the stored ids and rows and an edit, the ids and rows a FRESH build -- crag_index_add of the same rows in id
order -- would hold.  The GPU tests build a second index from this result and compare bit for bit."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def _check_table(ids: np.ndarray, rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[0] != ids.size:
        raise ValueError("one row per id")
    if np.any(np.diff(ids) <= 0):
        raise ValueError("stored ids ascend strictly")
    return ids, rows


def remove(ids, rows, drop_ids) -> Tuple[np.ndarray, np.ndarray, int]:
    """Rows whose id is listed leave (any order, repeats, absent ids ignored).  -> (ids, rows, removed)."""
    ids, rows = _check_table(ids, rows)
    keep = ~np.isin(ids, np.asarray(drop_ids, dtype=np.int64).reshape(-1))
    return ids[keep].copy(), rows[keep].copy(), int(ids.size - np.count_nonzero(keep))


def compact(ids, rows, keep) -> Tuple[np.ndarray, np.ndarray]:
    """Rows whose `keep` entry is false leave."""
    ids, rows = _check_table(ids, rows)
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    if keep.size != ids.size:
        raise ValueError("one keep entry per stored row")
    return ids[keep].copy(), rows[keep].copy()


def insert(ids, rows, new_ids, new_rows) -> Tuple[np.ndarray, np.ndarray]:
    """New rows (ids strictly ascending, none stored already) take their place in id order; ValueError otherwise,
    as the ABI answers CRAG_EINVAL with nothing changed."""
    ids, rows = _check_table(ids, rows)
    new_ids = np.asarray(new_ids, dtype=np.int64).reshape(-1)
    new_rows = np.asarray(new_rows, dtype=np.float32).reshape(new_ids.size, -1)
    if np.any(np.diff(new_ids) <= 0):
        raise ValueError("new ids ascend strictly")
    if np.any(np.isin(new_ids, ids)):
        raise ValueError("an id is stored already")
    if new_ids.size and rows.shape[0] and new_rows.shape[1] != rows.shape[1]:
        raise ValueError("row width")
    all_ids = np.concatenate([ids, new_ids])
    order = np.argsort(all_ids, kind="stable")
    all_rows = np.concatenate([rows.reshape(ids.size, new_rows.shape[1] if ids.size == 0 else rows.shape[1]), new_rows])
    return all_ids[order], all_rows[order]


def update(ids, rows, pos, new_rows) -> Tuple[np.ndarray, np.ndarray]:
    """crag_index_update: rows [pos, pos + n) take the new vectors, the ids stay.  The inputs are not modified;
    ValueError for a range outside the table, as the ABI answers CRAG_EINVAL with nothing changed."""
    ids, rows = _check_table(ids, rows)
    new_rows = np.asarray(new_rows, dtype=np.float32)
    if new_rows.ndim == 1:
        new_rows = new_rows[None, :]
    pos, n = int(pos), new_rows.shape[0]
    if pos < 0 or pos + n > ids.size:
        raise ValueError("update range outside the table")
    if n and new_rows.shape[1] != rows.shape[1]:
        raise ValueError("row width")
    ids, rows = ids.copy(), rows.copy()
    rows[pos:pos + n] = new_rows
    return ids, rows


def pack_keep(keep) -> np.ndarray:
    """The row_mask encoding of a keep array: bit (i & 7) of byte i >> 3, padded to whole 32-bit words."""
    k = np.asarray(keep, dtype=bool).reshape(-1)
    packed = np.packbits(k, bitorder="little")
    return np.pad(packed, (0, (-packed.size) % 4))
