"""Filter row masks built on the GPU -- the device counterpart of DenseTable.filter_mask, i.e. of the reference's
_build_filter_clause (app/retrieve.py:93-120), for up to 64 queries per launch (crag_filter_masks_host).

The filter columns of a table live in HBM beside its vectors (FilterColumns: call_started_at in microseconds and the
dense number of the row's call, 12 bytes per row); a request's predicates are compiled on the host into two date bounds
per query and, transposed, one 64-bit query set per CALL (compile_predicates: its cost is in the number of calls and
listed ids, never in the number of rows); the kernel evaluates them for every row and writes the packed masks the lanes
take.  DenseTable.filter_mask stays the public host form of the same predicate."""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from . import _native

MAX_QUERIES = _native.CRAG_FILTER_MAX_QUERIES
NO_LOWER = np.iinfo(np.int64).min   # date_from of a query without a lower bound; also a row's NULL / NaT timestamp
NO_UPPER = np.iinfo(np.int64).max   # date_to of a query without an upper bound


def mask_bytes(n_rows: int) -> int:
    """Bytes of one packed mask over n_rows rows (the minimal mask_stride)."""
    return ((int(n_rows) + 31) // 32) * 4


class FilterColumns:
    """The filter columns of one DenseTable: per row `started_us` (int64 microseconds since the epoch, NO_LOWER for
    NaT) and `call_slot` (int32: the dense number of the row's call in `slot_of`, numbered by first appearance), built in
    ONE host pass over the rows -- per table generation, not per request.  With a `device` the two arrays are uploaded
    (d_started_us, d_call_slot: 12 bytes per row of HBM); without one the object is plain arrays, which is all
    compile_predicates needs."""

    def __init__(self, call_started_at, call_ids, device=None, generation: Optional[int] = None) -> None:
        self.started_us = np.ascontiguousarray(np.asarray(call_started_at, dtype="datetime64[us]").astype(np.int64))
        self.n = int(self.started_us.size)
        if len(call_ids) != self.n:
            raise ValueError("call_started_at and call_ids must have one entry per row")
        slot_of: Dict[Any, int] = {}
        number = slot_of.setdefault
        self.call_slot = np.fromiter((number(c, len(slot_of)) for c in call_ids), dtype=np.int32, count=self.n)
        self.slot_of = slot_of
        self.n_calls = len(slot_of)
        self.generation = generation
        self.device = device
        self.d_started_us = self.d_call_slot = None
        self._slots: dict = {}   # per stream: ring of upload slots (the idiom of TechTokenIndex._slot)
        if device is not None:
            import torch
            self.d_started_us = torch.from_numpy(self.started_us).to(device)
            self.d_call_slot = torch.from_numpy(self.call_slot).to(device)

    def _slot(self, stream: int):
        import torch
        ring = self._slots.setdefault(stream, {"next": 0, "slots": []})
        if len(ring["slots"]) < 4:
            with torch.cuda.device(self.device):
                handle = _native.load().crag_upload_slot_create()
            if not handle:
                raise _native.NativeLibraryError(f"crag_upload_slot_create failed: {_native.last_error()}")
            ring["slots"].append(handle)
        slot = ring["slots"][ring["next"] % len(ring["slots"])]
        ring["next"] += 1
        return slot

    def close(self) -> None:
        rings, self._slots = getattr(self, "_slots", {}), {}
        for ring in rings.values():
            for handle in ring["slots"]:
                _native.load().crag_upload_slot_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone already
            pass

    def masks(self, qset: Optional[np.ndarray], date_from: np.ndarray, date_to: np.ndarray, stride: Optional[int] = None,
              out=None, stream: Optional[int] = None):
        """Enqueue the kernel for compiled predicates on `stream` (default: torch's current stream): a uint8 CUDA
        tensor [nq, stride] (stride: a multiple of 4 >= mask_bytes(n), default minimal), every byte written.  `out`: a
        tensor of that shape to write into (it may hold anything).  No host synchronisation."""
        import torch
        if self.device is None:
            raise _native.NativeLibraryError("these FilterColumns were built without a device")
        nq = int(date_from.size)
        if not 1 <= nq <= MAX_QUERIES or int(date_to.size) != nq:
            raise ValueError(f"a filter batch holds 1 to {MAX_QUERIES} queries")
        stride = mask_bytes(self.n) if stride is None else int(stride)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if out is None:
            from .fusion import _on_stream
            with _on_stream(stream, self.device):
                out = torch.empty((nq, stride), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (nq, stride) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 [{nq}, {stride}] tensor")
        if stride == 0:   # an empty table: the runs are empty
            return out
        date_from = np.ascontiguousarray(date_from, dtype=np.int64)
        date_to = np.ascontiguousarray(date_to, dtype=np.int64)
        qptr = None
        if qset is not None:
            qset = np.ascontiguousarray(qset, dtype=np.uint64)
            if qset.size != self.n_calls:
                raise ValueError("qset must have one word per call")
            qptr = (qset if qset.size else np.zeros(1, dtype=np.uint64)).ctypes.data   # (scoped, no calls: a valid address)
        rc = _native.load().crag_filter_masks_host(
            self.d_started_us.data_ptr() if self.n else None, self.d_call_slot.data_ptr() if self.n else None, self.n,
            self.n_calls, qptr, date_from.ctypes.data, date_to.ctypes.data, nq, self._slot(stream), out.data_ptr(), stride,
            ctypes.c_void_p(stream))
        _native.check(rc, "crag_filter_masks_host")
        return out


def _us(dt) -> int:
    from .retrieve import _naive_utc
    return int(np.datetime64(_naive_utc(dt), "us").astype(np.int64))


def compile_predicates(columns: FilterColumns, call_tags: Dict[Any, Sequence[str]],
                       batch: Sequence[Tuple[Any, Optional[Sequence[Any]]]]
                       ) -> Tuple[Optional[np.ndarray], np.ndarray, np.ndarray]:
    """batch: up to 64 (filters, call_ids) pairs, the arguments of DenseTable.filter_mask.  Returns (qset, date_from,
    date_to): uint64 [n_calls] or None when no query is call-scoped, int64 [nq] microseconds with NO_LOWER / NO_UPPER
    for an open side.  Semantics are filter_mask's, quirks included: nothing applies unless `filters` is truthy
    (call_ids too); call_ids == [] admits nothing; tags mean an overlap with call_tags[call], a call absent from
    call_tags has none; call ids and tags intersect; bounds go through _naive_utc."""
    nq = len(batch)
    if nq > MAX_QUERIES:
        raise ValueError(f"a filter batch holds at most {MAX_QUERIES} queries (got {nq}): the caller splits it")
    date_from = np.full(nq, NO_LOWER, dtype=np.int64)
    date_to = np.full(nq, NO_UPPER, dtype=np.int64)
    slot_of = columns.slot_of
    scoped: Dict[int, Sequence[int]] = {}
    for q, (filters, call_ids) in enumerate(batch):
        if not filters:
            continue
        if filters.date_from:
            date_from[q] = _us(filters.date_from)
        if filters.date_to:
            date_to[q] = _us(filters.date_to)
        admitted = None
        if call_ids is not None:
            admitted = {slot_of[c] for c in set(call_ids) if c in slot_of}
        if filters.call_tags:
            tags = set(filters.call_tags)
            tagged = {slot_of[c] for c, t in call_tags.items() if c in slot_of and tags.intersection(t or ())}
            admitted = tagged if admitted is None else (admitted & tagged)
        if admitted is not None:
            scoped[q] = sorted(admitted)
    if not scoped:
        return None, date_from, date_to
    open_bits = 0
    for q in range(nq):
        if q not in scoped:
            open_bits |= 1 << q
    qset = np.full(columns.n_calls, open_bits, dtype=np.uint64)
    for q, slots in scoped.items():
        if slots:
            qset[np.asarray(slots, dtype=np.int64)] |= np.uint64(1 << q)
    return qset, date_from, date_to


def is_unfiltered(qset: Optional[np.ndarray], date_from: np.ndarray, date_to: np.ndarray) -> bool:
    """No query of the compiled batch restricts anything (for one query: DenseTable.filter_mask returns None)."""
    return qset is None and bool(np.all(date_from == NO_LOWER)) and bool(np.all(date_to == NO_UPPER))
