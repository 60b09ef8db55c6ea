"""DenseIndex — the in-HBM replacement for the reference's `embedding vector(1024)` column and
its pgvector scan (reference: /root/reference/app/retrieve.py:326-389,
alembic/versions/0001_initial_schema.py:87).  Thin Python over the C ABI (include/crag_dense.h);
all arithmetic happens in the HIP library.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native

try:  # torch is plumbing only (device buffers / streams); numpy-only use works without it
    import torch
except Exception:  # pragma: no cover
    torch = None  # type: ignore


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _as_f32_2d(x, dim: int, what: str):
    """Return (pointer, rows, keepalive) for a [n, dim] float32 C-contiguous numpy/torch array."""
    if _is_torch(x):
        t = x
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        t = t.contiguous()
        if t.dim() != 2 or t.shape[1] != dim:
            raise ValueError(f"{what} must have shape [n, {dim}], got {tuple(t.shape)}")
        return t.data_ptr(), int(t.shape[0]), t
    a = np.asarray(x, dtype=np.float32)
    if a.ndim == 1:
        a = a[None, :]
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"{what} must have shape [n, {dim}], got {a.shape}")
    return a.ctypes.data, int(a.shape[0]), a


def _opt_ptr(t):
    """the device pointer of an optional tensor argument of the async wrappers (None: NULL)"""
    return None if t is None else t.data_ptr()


def _pad_lists(ids, cap: int, what: str = "", extra=None):
    """One flat list of ids or a sequence of ragged lists -> (single, lists, h_ids, counts): h_ids int64 [n_lists, width]
    padded with -1 (width = the longest list, at least 1; ValueError above `cap`, its text ending in `what`), counts
    int32 [n_lists].  extra: relevances shaped like ids; a fifth result is their float32 [n_lists, width], NaN padded."""
    single = len(ids) == 0 or np.ndim(ids[0]) == 0
    lists = [np.asarray(l, dtype=np.int64).reshape(-1) for l in ([ids] if single else ids)]
    extras = None
    if extra is not None:
        extras = [np.asarray(e, dtype=np.float32).reshape(-1) for e in ([extra] if single else extra)]
        if len(extras) != len(lists) or any(e.size != l.size for e, l in zip(extras, lists)):
            raise ValueError("ids and rel must have the same shape")
    width = max([int(l.size) for l in lists] + [1])
    if width > cap:
        raise ValueError(f"a list holds at most {cap} ids (got {width}){what}")
    h_ids = np.full((len(lists), width), -1, dtype=np.int64)
    for q, l in enumerate(lists):
        h_ids[q, :l.size] = l
    counts = np.asarray([l.size for l in lists], dtype=np.int32)
    if extras is None:
        return single, lists, h_ids, counts
    h_extra = np.full((len(lists), width), np.nan, dtype=np.float32)
    for q, e in enumerate(extras):
        h_extra[q, :e.size] = e
    return single, lists, h_ids, counts, h_extra


class DenseIndex:
    """Exact cosine top-k over fp32 rows resident in one GPU's HBM."""

    def __init__(self, dim: int = 1024, capacity: int = 1 << 20, device: int = 0) -> None:
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        self.dim = int(dim)
        self.device = int(device)
        self._mmr_scratch: dict = {}   # per (stream, nq, width): the scratch of mmr_async
        _native.check(self._lib.crag_index_create(self.device, self.dim, int(capacity),
                                                  ctypes.byref(self._h)), "crag_index_create")

    # -- lifecycle -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.crag_index_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._mmr_scratch = {}

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "DenseIndex":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __len__(self) -> int:
        return int(self._lib.crag_index_size(self._h))

    @property
    def capacity(self) -> int:
        return int(self._lib.crag_index_capacity(self._h))

    # -- corpus ----------------------------------------------------------------------------
    def add(self, vectors, ids=None) -> None:
        ptr, n, keep = _as_f32_2d(vectors, self.dim, "vectors")
        ids_ptr, keep_ids = None, None
        if ids is not None:
            if _is_torch(ids):
                keep_ids = ids.to(torch.int64).contiguous()
                if keep_ids.numel() != n:
                    raise ValueError("ids length mismatch")
                ids_ptr = keep_ids.data_ptr()
            else:
                keep_ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
                if keep_ids.size != n:
                    raise ValueError("ids length mismatch")
                ids_ptr = keep_ids.ctypes.data
        _native.check(self._lib.crag_index_add(self._h, ptr, ids_ptr, n), "crag_index_add")
        del keep, keep_ids

    def update(self, pos: int, vectors) -> None:
        ptr, n, keep = _as_f32_2d(vectors, self.dim, "vectors")
        _native.check(self._lib.crag_index_update(self._h, int(pos), ptr, n), "crag_index_update")
        del keep

    # -- in-place edits (crag_index_remove / compact / insert): afterwards the index is what a fresh build from the
    #    same rows in id order would be; each call waits for the searches in flight on this index ---------------
    @staticmethod
    def _ids_arg(ids, n: Optional[int] = None):
        """(pointer, count, keepalive) for int64 ids given as a numpy-like sequence or a torch tensor."""
        if _is_torch(ids):
            keep = ids.to(torch.int64).contiguous().reshape(-1)
            ptr, count = keep.data_ptr(), int(keep.numel())
        else:
            keep = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
            ptr, count = keep.ctypes.data, int(keep.size)
        if n is not None and count != n:
            raise ValueError("ids length mismatch")
        return (ptr if count else None), count, keep

    def remove(self, ids) -> int:
        """Remove the rows with these ids (any order, repeats and absent ids allowed; host sequence or CUDA
        tensor).  Returns the number of rows removed."""
        ptr, n, keep = self._ids_arg(ids)
        removed = ctypes.c_int64(0)
        _native.check(self._lib.crag_index_remove(self._h, ptr, n, ctypes.byref(removed)), "crag_index_remove")
        del keep
        return int(removed.value)

    def compact(self, keep) -> int:
        """Keep the rows whose entry of the bool array `keep` (one per stored row) is true, remove the others.
        Returns the new size."""
        k = np.asarray(keep, dtype=bool).reshape(-1)
        if k.size != len(self):
            raise ValueError(f"keep must have one entry per stored row ({len(self)}), got {k.size}")
        packed = self.pack_mask(k) if k.size else np.zeros((4,), dtype=np.uint8)
        size = ctypes.c_int64(0)
        _native.check(self._lib.crag_index_compact(self._h, packed.ctypes.data, ctypes.byref(size)), "crag_index_compact")
        return int(size.value)

    def insert(self, vectors, ids) -> None:
        """`add` for rows whose ids (strictly ascending) may lie between the stored ones: the rows behind them
        move up in place.  An id that is stored already is an error and leaves the index unchanged.  Takes host
        arrays or CUDA tensors like `add`."""
        ptr, n, keep = _as_f32_2d(vectors, self.dim, "vectors")
        ids_ptr, _, keep_ids = self._ids_arg(ids, n)
        _native.check(self._lib.crag_index_insert(self._h, ptr, ids_ptr, n), "crag_index_insert")
        del keep, keep_ids

    def get_rows(self, pos: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
        rows = np.empty((n, self.dim), dtype=np.float32)
        ids = np.empty((n,), dtype=np.int64)
        _native.check(self._lib.crag_index_get_rows(self._h, int(pos), int(n), rows.ctypes.data,
                                                    ids.ctypes.data), "crag_index_get_rows")
        return rows, ids

    def get_rows_into(self, pos: int, n: int, d_rows) -> np.ndarray:
        """Device-to-device form of get_rows: rows [pos, pos+n) into the float32 CUDA tensor d_rows
        ([n, dim], contiguous); returns their ids (host)."""
        if tuple(d_rows.shape) != (n, self.dim) or not d_rows.is_contiguous() or d_rows.dtype != torch.float32:
            raise ValueError(f"d_rows must be a contiguous float32 [{n}, {self.dim}] tensor")
        ids = np.empty((n,), dtype=np.int64)
        if n:
            _native.check(self._lib.crag_index_get_rows(self._h, int(pos), int(n), d_rows.data_ptr(),
                                                        ids.ctypes.data), "crag_index_get_rows")
        return ids

    @staticmethod
    def pack_mask(eligible) -> np.ndarray:
        """bool [n] or [nq, n] -> the bit mask the C ABI takes (bit i&7 of byte i>>3), with each
        row padded to a multiple of 4 bytes."""
        e = np.asarray(eligible, dtype=bool)
        packed = np.packbits(e, axis=-1, bitorder="little")
        pad = (-packed.shape[-1]) % 4
        if pad:
            width = [(0, 0)] * (packed.ndim - 1) + [(0, pad)]
            packed = np.pad(packed, width)
        return np.ascontiguousarray(packed)

    @staticmethod
    def _mask_arg(row_mask):
        """(pointer, array-like kept alive) of a packed mask given as numpy bytes or as a uint8 CUDA tensor (the C ABI
        detects the pointer kind).  A device mask must be complete in memory: the synchronous entries run on a stream
        of their own."""
        if _is_torch(row_mask):
            if row_mask.dtype != torch.uint8 or not row_mask.is_cuda or not row_mask.is_contiguous():
                raise ValueError("a tensor row_mask must be a contiguous uint8 CUDA tensor")
            return (row_mask.data_ptr() or None), row_mask
        row_mask = np.ascontiguousarray(np.asarray(row_mask, dtype=np.uint8))
        return row_mask.ctypes.data, row_mask

    def count_eligible(self, row_mask=None) -> int:
        """Rows a search could return under the (shared) mask: numpy bytes from pack_mask() or a uint8 CUDA tensor."""
        out = ctypes.c_int64(0)
        ptr = None
        if row_mask is not None:
            ptr, row_mask = self._mask_arg(row_mask)
            if row_mask.shape[-1] < ((len(self) + 31) // 32) * 4 and _is_torch(row_mask):
                raise ValueError("a device row_mask needs ceil(size/32)*4 bytes")
        _native.check(self._lib.crag_index_count_eligible(self._h, ptr, ctypes.byref(out)),
                      "crag_index_count_eligible")
        return int(out.value)

    # -- search ----------------------------------------------------------------------------
    def search(self, queries, k: int, row_mask=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Synchronous exact top-k.  Returns (ids [nq,k] int64 (-1 pad), scores [nq,k] float32
        (NaN pad), counts [nq] int32).  row_mask: packed bits from pack_mask() or a uint8 CUDA tensor in the same
        encoding (DenseTable.filter_mask_device; complete in memory), shape [bytes] (shared) or [nq, bytes] (per
        query)."""
        ptr, nq, keep = _as_f32_2d(queries, self.dim, "queries")
        if not 1 <= int(k) <= _native.CRAG_MAX_K:
            raise ValueError(f"k must be in [1, {_native.CRAG_MAX_K}] (got {k})")
        out_ids = np.empty((nq, k), dtype=np.int64)
        out_scores = np.empty((nq, k), dtype=np.float32)
        out_counts = np.empty((nq,), dtype=np.int32)
        mptr, stride = None, 0
        if row_mask is not None:
            mptr, row_mask = self._mask_arg(row_mask)
            need = ((len(self) + 31) // 32) * 4
            if row_mask.shape[-1] < need:
                raise ValueError(f"row_mask needs {need} bytes per row (use pack_mask)")
            if row_mask.ndim == 2:
                if row_mask.shape[0] != nq:
                    raise ValueError("per-query row_mask must have one row per query")
                stride = int(row_mask.shape[1])
                if stride % 4:
                    raise ValueError("row_mask row stride must be a multiple of 4 bytes")
        _native.check(self._lib.crag_index_search(self._h, ptr, nq, int(k), mptr, stride,
                                                  out_ids.ctypes.data, out_scores.ctypes.data,
                                                  out_counts.ctypes.data), "crag_index_search")
        del keep
        return out_ids, out_scores, out_counts

    def search_async(self, d_queries, k: int, d_out_ids, d_out_scores, d_out_counts,
                     d_row_mask=None, mask_stride: int = 0, stream: int = 0) -> None:
        """All-device search enqueued on `stream` (a hipStream_t as int, e.g.
        torch.cuda.current_stream().cuda_stream).  Arguments are torch CUDA tensors."""
        nq = int(d_queries.shape[0])
        _native.check(self._lib.crag_index_search_async(
            self._h, d_queries.data_ptr(), nq, int(k),
            _opt_ptr(d_row_mask), int(mask_stride),
            d_out_ids.data_ptr(), d_out_scores.data_ptr(), d_out_counts.data_ptr(),
            ctypes.c_void_p(stream)), "crag_index_search_async")

    def search_pipelined(self, d_queries, k: int, d_out_ids, d_out_scores, d_out_counts,
                         d_row_mask=None, mask_stride: int = 0, stream: int = 0, inputs_ready: bool = False) -> None:
        """Throughput form for a run of INDEPENDENT searches issued from one stream (crag_index_search_pipelined):
        consecutive calls rotate over three streams of the index's own (k <= 24; larger k runs in order), so search
        i + 1's preparation and scan run beside search i's selection.  The outputs are defined on `stream` only behind join(stream).  inputs_ready: the
        queries / mask are complete in memory now (no event orders the internal stream behind `stream`)."""
        nq = int(d_queries.shape[0])
        _native.check(self._lib.crag_index_search_pipelined(
            self._h, d_queries.data_ptr(), nq, int(k),
            _opt_ptr(d_row_mask), int(mask_stride),
            d_out_ids.data_ptr(), d_out_scores.data_ptr(), d_out_counts.data_ptr(),
            ctypes.c_void_p(stream), 1 if inputs_ready else 0), "crag_index_search_pipelined")

    def join(self, stream: int = 0) -> None:
        """Make `stream` wait for every pipelined search issued so far (does not block the host)."""
        _native.check(self._lib.crag_index_join(self._h, ctypes.c_void_p(stream)), "crag_index_join")

    # -- near-duplicate suppression (crag_index_dedupe_async) -------------------------------------
    def dedupe_async(self, d_ids, d_counts, threshold: float, d_out_ids, d_out_counts, d_out_dup_of=None,
                     d_out_sim=None, stream: int = 0) -> None:
        """Greedy near-duplicate suppression of ranked lists, enqueued on `stream`: d_ids int64 [nq, width <= 256]
        best first, d_counts int32 [nq] (the shape rrf_fuse emits).  An item is dropped iff a KEPT earlier item of its
        list has a cosine >= threshold with it (ids that are not stored, -1 and rows with a zero or non-finite norm are
        kept and suppress nothing).  d_out_ids [nq, width]: the kept ids in order, -1 padded; d_out_counts [nq];
        d_out_dup_of int32 / d_out_sim fp32 [nq, width] (optional): per input slot the slot that suppressed it (-1:
        kept) and that pair's cosine (NaN: kept).  Arguments are torch CUDA tensors."""
        if d_ids.dim() != 2:
            raise ValueError("d_ids must have shape [nq, width]")
        nq, width = int(d_ids.shape[0]), int(d_ids.shape[1])
        _native.check(self._lib.crag_index_dedupe_async(
            self._h, d_ids.data_ptr(), d_counts.data_ptr(), nq, width, float(threshold), d_out_ids.data_ptr(),
            d_out_counts.data_ptr(), _opt_ptr(d_out_dup_of), _opt_ptr(d_out_sim), ctypes.c_void_p(stream)),
            "crag_index_dedupe_async")

    def dedupe(self, ids, threshold: float):
        """Host convenience over dedupe_async for one ranked list of ids (a flat sequence) or several (a sequence of
        sequences, lengths may differ; at most 256 ids each).  Returns (keep_slots, dup_of, sim): the input slots that
        are kept (int64, ascending), per input slot the slot that suppressed it (-1: kept) and that pair's cosine
        (NaN: kept) -- arrays for one list, lists of arrays for several.  Synchronises."""
        if torch is None:  # pragma: no cover
            raise _native.NativeLibraryError("DenseIndex.dedupe stages its buffers with torch")
        single, lists, h_ids, counts = _pad_lists(ids, _native.CRAG_DEDUPE_MAX_WIDTH)
        dev = torch.device("cuda", self.device)
        d_ids, d_ct = torch.from_numpy(h_ids).to(dev), torch.from_numpy(counts).to(dev)
        d_out = torch.empty_like(d_ids)
        d_oct = torch.empty_like(d_ct)
        d_dup = torch.empty(h_ids.shape, dtype=torch.int32, device=dev)
        d_sim = torch.empty(h_ids.shape, dtype=torch.float32, device=dev)
        self.dedupe_async(d_ids, d_ct, threshold, d_out, d_oct, d_dup, d_sim,
                          stream=torch.cuda.current_stream(dev).cuda_stream)
        dup, sim = d_dup.cpu().numpy(), d_sim.cpu().numpy()
        res = [(np.flatnonzero(dup[q, :l.size] < 0).astype(np.int64), dup[q, :l.size].copy(), sim[q, :l.size].copy())
               for q, l in enumerate(lists)]
        if single:
            return res[0]
        return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]

    # -- exact top-k and scores over listed rows (crag_index_search_ids_async) ----------------------
    @staticmethod
    def search_ids_scratch_bytes(nq: int, width: int) -> int:
        return int(_native.load().crag_index_search_ids_scratch_bytes(int(nq), int(width)))

    def search_ids_async(self, d_queries, d_ids, d_counts, k: int, d_out_ids, d_out_scores, d_out_counts,
                         d_out_slot_scores=None, shared: bool = False, scratch=None, stream: int = 0) -> None:
        """The search of `search_async` over LISTED rows only, enqueued on `stream`: d_ids int64 [nq, width <= 4096]
        (shared=True: one [width] list for every query), d_counts int32 [nq] ([1] when shared).  The outputs are what
        search_async returns under a mask of the listed ids' positions, bit for bit; d_out_slot_scores fp32
        [nq, width] (optional) receives the score of every input slot (NaN: beyond the count or ignored).  scratch: a
        uint8 CUDA tensor of search_ids_scratch_bytes(nq, width) bytes, one per stream in use (default: allocated
        here).  Arguments are torch CUDA tensors."""
        nq = int(d_queries.shape[0])
        if d_ids.dim() != (1 if shared else 2) or (not shared and int(d_ids.shape[0]) != nq):
            raise ValueError("d_ids must have shape [nq, width], or [width] with shared=True")
        width = int(d_ids.shape[-1])
        if scratch is None:
            scratch = torch.empty(self.search_ids_scratch_bytes(nq, width), dtype=torch.uint8, device=d_ids.device)
        _native.check(self._lib.crag_index_search_ids_async(
            self._h, d_queries.data_ptr(), nq, d_ids.data_ptr(), d_counts.data_ptr(), width, 0 if shared else width,
            int(k), d_out_ids.data_ptr(), d_out_scores.data_ptr(), d_out_counts.data_ptr(),
            _opt_ptr(d_out_slot_scores), scratch.data_ptr(),
            int(scratch.numel()) * scratch.element_size(), ctypes.c_void_p(stream)), "crag_index_search_ids_async")

    def search_ids(self, queries, ids, k: int, slot_scores: bool = False):
        """Host convenience over search_ids_async: exact top-k of every query among the listed ids -- one flat list
        shared by all queries, or one list per query (lengths may differ; at most 4096 ids each, ValueError above:
        use a row_mask).  Returns numpy (ids [nq, k], scores [nq, k], counts [nq]) as `search` does, and with
        slot_scores=True also [nq, width] scores per input slot (NaN: pad or ignored id).  Synchronises."""
        if torch is None:  # pragma: no cover
            raise _native.NativeLibraryError("DenseIndex.search_ids stages its buffers with torch")
        ptr, nq, keep = _as_f32_2d(queries, self.dim, "queries")
        if not 1 <= int(k) <= _native.CRAG_MAX_K:
            raise ValueError(f"k must be in [1, {_native.CRAG_MAX_K}] (got {k})")
        if len(ids) and np.ndim(ids[0]) != 0 and len(ids) != nq:
            raise ValueError("per-query id lists must have one list per query")
        shared, _, h_ids, counts = _pad_lists(ids, _native.CRAG_SUBSET_MAX_WIDTH, ": use a row_mask")
        width = h_ids.shape[1]
        dev = torch.device("cuda", self.device)
        d_q = keep.to(dev) if _is_torch(keep) else torch.from_numpy(keep).to(dev)
        d_ids = torch.from_numpy(h_ids[0] if shared else h_ids).to(dev)
        d_ct = torch.from_numpy(counts).to(dev)
        out_ids = torch.empty(nq, int(k), dtype=torch.int64, device=dev)
        out_sc = torch.empty(nq, int(k), dtype=torch.float32, device=dev)
        out_ct = torch.empty(nq, dtype=torch.int32, device=dev)
        slot = torch.empty(nq, width, dtype=torch.float32, device=dev) if slot_scores else None
        if nq:
            self.search_ids_async(d_q, d_ids, d_ct, k, out_ids, out_sc, out_ct, slot, shared=shared,
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
        res = (out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_ct.cpu().numpy())
        return res + (slot.cpu().numpy(),) if slot_scores else res

    # -- maximal marginal relevance over ranked lists (crag_index_mmr_async) ------------------------
    @staticmethod
    def mmr_scratch_bytes(nq: int, width: int) -> int:
        return int(_native.load().crag_index_mmr_scratch_bytes(int(nq), int(width)))

    def mmr_async(self, d_ids, d_rel, d_counts, lam: float, k: int, d_out_ids, d_out_rel, d_out_counts,
                  d_out_value=None, d_out_slots=None, d_out_sim_rows=None, scratch=None, stream: int = 0) -> None:
        """MMR over ranked lists, enqueued on `stream`: d_ids int64 / d_rel fp32 [nq, width <= 256], d_counts int32 [nq]
        (what search_async emits).  k times per list the candidate with the largest lam * rel - (1 - lam) * pen is
        picked (ties: the lower id), pen being the largest cosine to a row picked before; slots beyond the count, -1, a
        non-finite rel and a repeated id are ignored, an id without a stored vector is picked by rel alone.  d_out_ids
        int64 / d_out_rel fp32 [nq, k] in pick order (-1 / NaN pad), d_out_counts int32 [nq]; optional d_out_value fp32
        and d_out_slots int32 [nq, k], d_out_sim_rows fp32 [nq, k, width] (cos(pick, slot), NaN: no pair).  scratch: a
        uint8 CUDA tensor of mmr_scratch_bytes(nq, width) bytes, one per stream in use (default: kept here per (stream,
        nq, width)).  Arguments are torch CUDA tensors."""
        if d_ids.dim() != 2:
            raise ValueError("d_ids must have shape [nq, width]")
        nq, width = int(d_ids.shape[0]), int(d_ids.shape[1])
        if scratch is None:
            scratch = self._mmr_scratch.get((stream, nq, width))
            if scratch is None:
                scratch = self._mmr_scratch[(stream, nq, width)] = torch.empty(
                    self.mmr_scratch_bytes(nq, width), dtype=torch.uint8, device=d_ids.device)
        _native.check(self._lib.crag_index_mmr_async(
            self._h, d_ids.data_ptr(), d_rel.data_ptr(), d_counts.data_ptr(), nq, width, float(lam), int(k),
            d_out_ids.data_ptr(), d_out_rel.data_ptr(), _opt_ptr(d_out_value), _opt_ptr(d_out_slots),
            _opt_ptr(d_out_sim_rows), d_out_counts.data_ptr(), scratch.data_ptr(), int(scratch.numel()) * scratch.element_size(),
            ctypes.c_void_p(stream)), "crag_index_mmr_async")

    def mmr(self, ids, rel, lam: float, k: int):
        """Host convenience over mmr_async for one list (flat sequences of ids and relevances) or several (sequences of
        sequences, lengths may differ; at most 256 slots each).  Returns (ids, rel, value, slots) of the picks in pick
        order -- arrays for one list, lists of arrays for several.  Synchronises."""
        if torch is None:  # pragma: no cover
            raise _native.NativeLibraryError("DenseIndex.mmr stages its buffers with torch")
        single, lists, h_ids, counts, h_rel = _pad_lists(ids, _native.CRAG_MMR_MAX_WIDTH, extra=rel)
        if not 1 <= int(k) <= _native.CRAG_MMR_MAX_WIDTH:
            raise ValueError(f"k must be in [1, {_native.CRAG_MMR_MAX_WIDTH}] (got {k})")
        if not 0.0 <= float(lam) <= 1.0:
            raise ValueError(f"lam must be finite, in [0, 1] (got {lam})")
        nq, k = len(lists), int(k)
        dev = torch.device("cuda", self.device)
        d_ids, d_rel, d_ct = (torch.from_numpy(a).to(dev) for a in (h_ids, h_rel, counts))
        o_ids = torch.empty(nq, k, dtype=torch.int64, device=dev)
        o_rel = torch.empty(nq, k, dtype=torch.float32, device=dev)
        o_val = torch.empty(nq, k, dtype=torch.float32, device=dev)
        o_slot = torch.empty(nq, k, dtype=torch.int32, device=dev)
        o_ct = torch.empty(nq, dtype=torch.int32, device=dev)
        if nq:
            self.mmr_async(d_ids, d_rel, d_ct, lam, k, o_ids, o_rel, o_ct, o_val, o_slot,
                           stream=torch.cuda.current_stream(dev).cuda_stream)
        ct = o_ct.cpu().numpy()
        outs = [t.cpu().numpy() for t in (o_ids, o_rel, o_val, o_slot)]
        res = [tuple(a[q, :ct[q]].copy() for a in outs) for q in range(nq)]
        if single:
            return res[0]
        return tuple([r[i] for r in res] for i in range(4))

    # -- exact top-k under a cap per group (crag_index_search_grouped_async) ------------------------
    GROUPED_SCRATCH_LIMIT = 256 << 20   # search_grouped splits its queries so that the scratch stays at or below this

    @staticmethod
    def search_grouped_scratch_bytes(nq: int, n_groups: int, per_group: int) -> int:
        return int(_native.load().crag_index_search_grouped_scratch_bytes(int(nq), int(n_groups), int(per_group)))

    def search_grouped_async(self, d_queries, k: int, d_row_group, n_groups: int, per_group: int, d_out_ids,
                             d_out_scores, d_out_counts, d_out_groups=None, d_row_mask=None, mask_stride: int = 0,
                             scratch=None, stream: int = 0) -> None:
        """The search of `search_async` with at most `per_group` rows per group, enqueued on `stream`: d_row_group int32
        [size] by row position (a number outside [0, n_groups): the row is ignored).  Per query the eligible rows are
        walked best first and a row is kept iff its group holds fewer than per_group kept rows, up to k; scores are the
        bits search_async returns.  d_out_groups int32 [nq, k] (optional, -1 pad).  scratch: a uint8 CUDA tensor of
        search_grouped_scratch_bytes(nq, n_groups, per_group) bytes, one per stream in use, contents arbitrary
        (default: allocated here).  Arguments are torch CUDA tensors."""
        nq = int(d_queries.shape[0])
        if scratch is None:
            scratch = torch.empty(self.search_grouped_scratch_bytes(nq, n_groups, per_group), dtype=torch.uint8,
                                  device=d_queries.device)
        _native.check(self._lib.crag_index_search_grouped_async(
            self._h, d_queries.data_ptr(), nq, int(k), d_row_group.data_ptr(), int(n_groups), int(per_group),
            _opt_ptr(d_row_mask), int(mask_stride), d_out_ids.data_ptr(),
            d_out_scores.data_ptr(), _opt_ptr(d_out_groups), d_out_counts.data_ptr(),
            scratch.data_ptr(), int(scratch.numel()) * scratch.element_size(), ctypes.c_void_p(stream)),
            "crag_index_search_grouped_async")

    def search_grouped(self, queries, k: int, row_group, n_groups: int, per_group: int, row_mask=None):
        """Host convenience over search_grouped_async.  queries / row_group ([size] int32) / row_mask (packed bits from
        pack_mask(), [bytes] shared or [nq, bytes] per query) may be numpy arrays or CUDA tensors.  Returns numpy
        (ids [nq, k], scores [nq, k], groups [nq, k], counts [nq]); the queries are split so that the scratch of one
        call stays at or below GROUPED_SCRATCH_LIMIT (a single query may exceed it).  Synchronises."""
        if torch is None:  # pragma: no cover
            raise _native.NativeLibraryError("DenseIndex.search_grouped stages its buffers with torch")
        _, nq, keep = _as_f32_2d(queries, self.dim, "queries")
        k, n_groups, per_group = int(k), int(n_groups), int(per_group)
        if not 1 <= k <= _native.CRAG_MAX_K:
            raise ValueError(f"k must be in [1, {_native.CRAG_MAX_K}] (got {k})")
        if not 1 <= per_group <= _native.CRAG_GROUP_MAX_PER:
            raise ValueError(f"per_group must be in [1, {_native.CRAG_GROUP_MAX_PER}] (got {per_group})")
        if not 1 <= n_groups < 1 << 31:
            raise ValueError(f"n_groups must be in [1, 2^31) (got {n_groups})")
        if nq == 0 or len(self) == 0:   # nothing to rank: the pads of the C ABI
            return (np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), np.nan, dtype=np.float32),
                    np.full((nq, k), -1, dtype=np.int32), np.zeros((nq,), dtype=np.int32))
        dev = torch.device("cuda", self.device)

        def on_device(x, dtype):
            t = x if _is_torch(x) else torch.from_numpy(np.ascontiguousarray(x))
            return t.to(device=dev, dtype=dtype).contiguous()

        d_q = on_device(keep, torch.float32)
        d_grp = on_device(row_group, torch.int32).reshape(-1)
        if int(d_grp.numel()) != len(self):
            raise ValueError(f"row_group needs one entry per stored row ({len(self)}, got {int(d_grp.numel())})")
        d_mask, stride = None, 0
        if row_mask is not None:
            d_mask = on_device(row_mask, torch.uint8)
            need = ((len(self) + 31) // 32) * 4
            if d_mask.shape[-1] < need:
                raise ValueError(f"row_mask needs {need} bytes per row (use pack_mask)")
            if d_mask.dim() == 2:
                if d_mask.shape[0] != nq:
                    raise ValueError("per-query row_mask must have one row per query")
                stride = int(d_mask.shape[1])
                if stride % 4:
                    raise ValueError("row_mask row stride must be a multiple of 4 bytes")
        out_ids = torch.empty(nq, k, dtype=torch.int64, device=dev)
        out_sc = torch.empty(nq, k, dtype=torch.float32, device=dev)
        out_grp = torch.empty(nq, k, dtype=torch.int32, device=dev)
        out_ct = torch.empty(nq, dtype=torch.int32, device=dev)
        per_query = self.search_grouped_scratch_bytes(2, n_groups, per_group) - \
            self.search_grouped_scratch_bytes(1, n_groups, per_group)
        step = max(1, min(65535, self.GROUPED_SCRATCH_LIMIT // max(per_query + 8, 1)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        scratch = None
        for q0 in range(0, nq, step):
            q1 = min(nq, q0 + step)
            if scratch is None:
                scratch = torch.empty(self.search_grouped_scratch_bytes(q1 - q0, n_groups, per_group), dtype=torch.uint8,
                                      device=dev)
            self.search_grouped_async(d_q[q0:q1], k, d_grp, n_groups, per_group, out_ids[q0:q1], out_sc[q0:q1],
                                      out_ct[q0:q1], out_grp[q0:q1],
                                      d_row_mask=None if d_mask is None else (d_mask[q0:q1] if stride else d_mask),
                                      mask_stride=stride, scratch=scratch, stream=stream)
        return out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_grp.cpu().numpy(), out_ct.cpu().numpy()

    # -- profiling / reporting -------------------------------------------------------------
    def profile_enable(self, every: int = 1) -> None:
        """Record HIP events around the scan/merge kernels of every `every`-th search (0 = off)."""
        _native.check(self._lib.crag_index_profile_enable(self._h, int(every)), "profile_enable")

    def profile_read(self) -> Tuple[int, float, float]:
        n = ctypes.c_int64(0)
        scan = ctypes.c_double(0.0)
        merge = ctypes.c_double(0.0)
        _native.check(self._lib.crag_index_profile_read(self._h, ctypes.byref(n), ctypes.byref(scan),
                                                        ctypes.byref(merge)), "profile_read")
        return int(n.value), float(scan.value), float(merge.value)

    def profile_read_ex(self) -> Tuple[int, float, float, float]:
        """(samples, scan ms total, rest ms total, back-to-back event pair ms total): see crag_index_profile_read_ex."""
        n = ctypes.c_int64(0)
        scan, merge, pair = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        _native.check(self._lib.crag_index_profile_read_ex(self._h, ctypes.byref(n), ctypes.byref(scan),
                                                           ctypes.byref(merge), ctypes.byref(pair)), "profile_read_ex")
        return int(n.value), float(scan.value), float(merge.value), float(pair.value)

    def prefilter_stats(self) -> dict:
        """Searches / candidates / exactly rescored rows of the prefilter path since the last call."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _native.check(self._lib.crag_index_prefilter_stats(self._h, ctypes.byref(a), ctypes.byref(b),
                                                           ctypes.byref(c)), "prefilter_stats")
        return {"searches": a.value, "candidates": b.value, "rescored_rows": c.value}

    def phase_trace(self):
        """Developer probe (CRAG_PHASE_TRACE=1 when the index was created): see crag_index_phase_trace."""
        buf = (ctypes.c_uint64 * 128)()
        _native.check(self._lib.crag_index_phase_trace(self._h, buf), "phase_trace")
        return [int(v) for v in buf]

    def prefilter_row_bytes(self) -> int:
        """Bytes of one corpus row the prefilter scan streams (2 KiB with the fp16 mirror, 4 KiB without, 0 = off)."""
        return int(self._lib.crag_index_prefilter_row_bytes(self._h))

    def last_scan_kernel(self) -> str:
        """Name of the scan kernel the most recent search launched (as rocprofv3 prints it)."""
        name = self._lib.crag_index_last_scan_kernel(self._h)
        return name.decode() if name else ""

    def scan_waits(self) -> str:
        """Wait schedule of the most recent scan's corpus loads: "fragment" or "tile" (see crag_index_scan_waits)."""
        name = self._lib.crag_index_scan_waits(self._h)
        return name.decode() if name else ""

    def scan_geometry(self, nq: int) -> dict:
        wg, th, qb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        ab = ctypes.c_int64(0)
        _native.check(self._lib.crag_index_scan_geometry(self._h, int(nq), ctypes.byref(wg),
                                                         ctypes.byref(th), ctypes.byref(qb),
                                                         ctypes.byref(ab)), "scan_geometry")
        return {"workgroups": wg.value, "threads": th.value, "query_blocks": qb.value,
                "algorithmic_bytes": int(ab.value)}


def merge_topk(d_ids, d_scores, d_counts, d_out_ids, d_out_scores, d_out_counts, stream: int = 0,
               device: Optional[int] = None) -> None:
    """Merge [n_lists, nq, k] per-shard results (torch CUDA tensors) into [nq, k] on the GPU."""
    lib = _native.load()
    n_lists, nq, k = (int(v) for v in d_ids.shape)
    dev = d_ids.device.index if device is None else device
    _native.check(lib.crag_merge_topk(int(dev or 0), d_ids.data_ptr(), d_scores.data_ptr(),
                                      d_counts.data_ptr(), n_lists, nq, k, d_out_ids.data_ptr(),
                                      d_out_scores.data_ptr(), d_out_counts.data_ptr(),
                                      ctypes.c_void_p(stream)), "crag_merge_topk")


class ResultRecord:
    """One rank's search output packed for a single all-gather: a uint8 CUDA buffer with typed views
    (ids int64 [nq,k], scores fp32 [nq,k], counts int32 [nq]) laid out as crag_merge_topk_packed
    expects."""

    @staticmethod
    def record_bytes(nq: int, k: int) -> int:
        return int(_native.load().crag_result_record_bytes(int(nq), int(k)))

    def __init__(self, nq: int, k: int, device, buf=None) -> None:
        """buf: an existing uint8 tensor of record_bytes(nq, k) bytes to lay the record over (this rank's slot of an
        all-gather buffer: the collective then runs in place); default: a buffer of its own."""
        self.nq, self.k = int(nq), int(k)
        self.nbytes = self.record_bytes(self.nq, self.k)
        if buf is None:
            buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        if buf.dtype != torch.uint8 or buf.numel() != self.nbytes or not buf.is_contiguous() or buf.data_ptr() % 8:
            raise ValueError("a ResultRecord needs a contiguous, 8-byte aligned uint8 buffer of record_bytes(nq, k) bytes")
        self.buf = buf
        a, b = self.nq * self.k * 8, self.nq * self.k * 12
        self.ids = self.buf[:a].view(torch.int64).view(self.nq, self.k)
        self.scores = self.buf[a:b].view(torch.float32).view(self.nq, self.k)
        self.counts = self.buf[b:b + self.nq * 4].view(torch.int32)


def merge_topk_packed(d_records, n_lists: int, nq: int, k: int, d_out_ids, d_out_scores, d_out_counts,
                      stream: int = 0) -> None:
    """Merge n_lists gathered ResultRecords (one contiguous uint8 CUDA tensor) into [nq, k]."""
    lib = _native.load()
    _native.check(lib.crag_merge_topk_packed(int(d_records.device.index or 0), d_records.data_ptr(), int(n_lists),
                                             int(nq), int(k), d_out_ids.data_ptr(), d_out_scores.data_ptr(),
                                             d_out_counts.data_ptr(), ctypes.c_void_p(stream)),
                  "crag_merge_topk_packed")
