"""Character-trigram field of the BM25 lane -- what the reference gets from the `pdb.ngram(3,3)` aliases of its pg_search
indexes (alembic/versions/0005_add_bm25_ngram.py, 0006_add_artifact_chunks.py; "BM25 ngram robustness (ASR noise)",
PHASED_PLAN.md:113): a misspelt or mis-transcribed query word still shares most of its 3-grams with the intended one.

NOT parity with Tantivy's ngram tokenizer: the rule is this tree's own (include/crag_dense.h, crag_ngram_extract;
DESIGN.md 4.7b lists the departures).  In short, over the BYTES of one row: decode UTF-8 leniently (a malformed byte is a
separator of one byte), fold A-Z, keep ASCII letters and digits and everything >= 0x80 as gram characters, and emit one
gram per three consecutive gram characters: key = cp0 << 42 | cp1 << 21 | cp2.  dl = the row's number of grams, tf
saturates at 65 535, and the term id of a key is its rank among the index's distinct keys.

`ngram_keys_host` / `ngram_csr_host` are the rule in plain Python and numpy (the oracle of the build); `NgramIndex` builds
the same arrays on the GPU (csrc/crag_ngram.hip around torch.sort and torch.cumsum) and scores them with the word lane's
kernels (crag_bm25_lane_host): same formula, this field's N, df and avgdl."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from . import _native
from .bm25 import K1, TF_MAX, Bm25Index

TILE_BYTES = _native.CRAG_NGRAM_TILE   # bytes of text per workgroup of the extraction kernel (CRAG_NGRAM_TILE)
NO_KEY = 2**63 - 1                     # the slot of a byte position where no gram starts (CRAG_NGRAM_NO_KEY)
MAX_TEXT_BYTES = 2**31 - 1             # one index; a larger corpus is split by rows into several


def ngram_keys_host(data: bytes) -> List[int]:
    """The keys of the grams of one row's bytes, in order of their start position (the rule, sequentially)."""
    data = bytes(data)
    n = len(data)
    chars: List[int] = []          # folded gram characters, -1 for a separator
    i = 0
    while i < n:
        b = data[i]
        length, cp = 1, b
        if b >= 0x80:
            length = 2 if 0xC0 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF7 else 0
            ok = length > 0 and i + length <= n and all(data[i + j] & 0xC0 == 0x80 for j in range(1, length))
            if ok:
                cp = b & (0xFF >> (length + 1))
                for j in range(1, length):
                    cp = (cp << 6) | (data[i + j] & 0x3F)
                ok = cp <= 0x10FFFF
            if not ok:             # malformed, cut off, F8..FF or a stray continuation: one separator of one byte
                chars.append(-1)
                i += 1
                continue
        if 0x41 <= cp <= 0x5A:
            cp += 0x20
        chars.append(cp if cp >= 0x80 or 0x30 <= cp <= 0x39 or 0x61 <= cp <= 0x7A else -1)
        i += length
    return [(a << 42) | (b << 21) | c for a, b, c in zip(chars, chars[1:], chars[2:]) if a >= 0 and b >= 0 and c >= 0]


def ngram_keys(text: str) -> List[int]:
    """The rule over the text's UTF-8 bytes (a lone surrogate becomes '?')."""
    return ngram_keys_host((text or "").encode("utf-8", "replace"))


def ngram_csr_host(rows_bytes: Sequence[bytes]) -> Dict[str, np.ndarray]:
    """The index of these rows by the rule: keys int64 [V] ascending, post_ptr int64 [V + 1], post_pos int32 [nnz]
    (ascending inside a term), post_tf uint16 [nnz] (saturated), doc_len int32 [N]."""
    n = len(rows_bytes)
    doc_len = np.zeros(n, dtype=np.int32)
    all_keys, all_rows = [], []
    for r, data in enumerate(rows_bytes):
        ks = ngram_keys_host(data)
        doc_len[r] = len(ks)
        if ks:
            all_keys.append(np.asarray(ks, dtype=np.int64))
            all_rows.append(np.full(len(ks), r, dtype=np.int64))
    if not all_keys:
        return {"keys": np.empty(0, np.int64), "post_ptr": np.zeros(1, np.int64), "post_pos": np.empty(0, np.int32),
                "post_tf": np.empty(0, np.uint16), "doc_len": doc_len}
    gk, gr = np.concatenate(all_keys), np.concatenate(all_rows)
    order = np.lexsort((gr, gk))
    gk, gr = gk[order], gr[order]
    head = np.ones(gk.size, dtype=bool)
    head[1:] = (gk[1:] != gk[:-1]) | (gr[1:] != gr[:-1])
    first = np.flatnonzero(head)
    tf = np.diff(np.append(first, gk.size))
    pk = gk[first]
    keys, df = np.unique(pk, return_counts=True)
    post_ptr = np.zeros(keys.size + 1, dtype=np.int64)
    np.cumsum(df, out=post_ptr[1:])
    return {"keys": keys, "post_ptr": post_ptr, "post_pos": gr[first].astype(np.int32),
            "post_tf": np.minimum(tf, TF_MAX).astype(np.uint16), "doc_len": doc_len}


def query_terms_host(keys: np.ndarray, df: np.ndarray, n_rows: int, query_texts: Sequence):
    """Queries (str, or bytes as they are) -> (q_ptr int32 [nq + 1], term ids int32 ascending inside a query, weights
    fp32) for an index with these `keys` (ascending) and `df`: the query's grams, counted; a gram the index does not
    hold is dropped; weight = qtf * idf * (k1 + 1) with idf = ln(1 + (N - df + 0.5) / (df + 0.5)) in fp64, rounded once."""
    q_ptr = np.zeros(len(query_texts) + 1, dtype=np.int32)
    terms, qtfs = [], []
    for q, text in enumerate(query_texts):
        data = text if isinstance(text, (bytes, bytearray)) else (text or "").encode("utf-8", "replace")
        ks, counts = np.unique(np.asarray(ngram_keys_host(data), dtype=np.int64), return_counts=True)
        at = np.searchsorted(keys, ks)
        known = at < keys.size
        known[known] = keys[at[known]] == ks[known]
        terms.append(at[known].astype(np.int32))     # keys ascend, so the ids do
        qtfs.append(counts[known].astype(np.float64))
        q_ptr[q + 1] = q_ptr[q] + int(known.sum())
    term_ids = np.concatenate(terms) if terms else np.empty(0, dtype=np.int32)
    qtf = np.concatenate(qtfs) if qtfs else np.empty(0, dtype=np.float64)
    dfq = np.asarray(df)[term_ids].astype(np.float64)
    weights = qtf * np.log(1.0 + (float(n_rows) - dfq + 0.5) / (dfq + 0.5)) * (K1 + 1.0)
    return q_ptr, term_ids.astype(np.int32), weights.astype(np.float32)   # fp64 up to here, rounded once


class NgramIndex(Bm25Index):
    """The trigram field of a text column: the rows' bytes on the host (the source of truth, kept for `extend`), the
    inverted CSR on the device, a host copy of `keys` and `df` for query preparation.  `search` / `search_terms`, the
    upload slots and `close` are Bm25Index's: the same kernels score both fields."""

    def __init__(self, texts: Sequence[str], ids: Sequence[int], device) -> None:
        self._init_rows([(t or "").encode("utf-8", "replace") for t in texts], ids, device)

    @classmethod
    def from_bytes(cls, rows_bytes: Sequence[bytes], ids: Sequence[int], device) -> "NgramIndex":
        """An index over rows given as bytes (any bytes: the rule defines what malformed UTF-8 yields)."""
        self = cls.__new__(cls)
        self._init_rows(rows_bytes, ids, device)
        return self

    def _init_rows(self, rows_bytes, ids, device) -> None:
        import torch
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.text = np.empty(0, dtype=np.uint8)
        self.text_ptr = np.zeros(1, dtype=np.int64)
        self.ids = np.empty(0, dtype=np.int64)
        self._ring = _native.UploadRing(self.device)
        self._buffers = {}
        self._append(rows_bytes, ids)
        self._build()

    # ---- host side ---------------------------------------------------------------------------------------------
    def _append(self, rows_bytes, ids) -> None:
        new_ids = np.asarray(list(ids), dtype=np.int64).reshape(-1)
        rows_bytes = [bytes(r) for r in rows_bytes]
        if len(rows_bytes) != new_ids.size:
            raise ValueError("rows and ids must have one entry per row")
        prev = self.ids[-1] if self.ids.size else None
        if (new_ids.size and prev is not None and new_ids[0] <= prev) or np.any(np.diff(new_ids) <= 0):
            raise ValueError("ids must ascend with the row position (and continue above the stored ids)")
        if self.ids.size + new_ids.size > 2**31 - 1:
            raise ValueError("the lane addresses rows with 31 bits")
        lens = np.fromiter((len(r) for r in rows_bytes), dtype=np.int64, count=len(rows_bytes))
        if self.text.size + int(lens.sum()) > MAX_TEXT_BYTES:
            raise ValueError("one trigram index holds at most 2^31 - 1 bytes of text: split the corpus by rows")
        self.text = np.concatenate([self.text, np.frombuffer(b"".join(rows_bytes), dtype=np.uint8)])
        self.text_ptr = np.concatenate([self.text_ptr, self.text_ptr[-1] + np.cumsum(lens)])
        self.ids = np.concatenate([self.ids, new_ids])

    def _build(self) -> None:
        """Upload the bytes and build keys, post_ptr, post_pos, post_tf and doc_len on the device (crag_ngram_* around a
        stable sort of the slots by key and one prefix sum).  Waits for the device: the sizes V and nnz come back."""
        import torch
        lib = _native.load()
        dev, n, n_bytes = self.device, int(self.ids.size), int(self.text.size)

        def empty(size, dtype):
            return torch.empty(max(int(size), 1), dtype=dtype, device=dev)    # (a valid address for empty arrays)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            d_text = torch.from_numpy(self.text).to(dev) if n_bytes else empty(16, torch.uint8)
            d_ptr = torch.from_numpy(self.text_ptr).to(dev)
            need = int(lib.crag_ngram_scratch_bytes(n_bytes, n))
            if need < 0:
                raise _native.NativeLibraryError(f"crag_ngram_scratch_bytes({n_bytes}, {n}) failed (code {need})")
            scratch = empty(need // 8, torch.int64)
            slot_keys, slot_rows, d_doc_len = empty(n_bytes, torch.int64), empty(n_bytes, torch.int32), empty(n, torch.int32)
            _native.check(lib.crag_ngram_extract(d_text.data_ptr(), n_bytes, d_ptr.data_ptr(), n, slot_keys.data_ptr(),
                                                 slot_rows.data_ptr(), d_doc_len.data_ptr(), scratch.data_ptr(),
                                                 scratch.numel() * 8, stream), "crag_ngram_extract")
            grams = int(d_doc_len[:n].sum(dtype=torch.int64)) if n else 0
            # torch.sort(stable=True) keeps equal keys in slot order, and slots are in text order: rows ascend in a key
            sorted_keys, sorted_rows = empty(0, torch.int64), empty(0, torch.int32)
            if grams:
                sorted_keys, order = torch.sort(slot_keys[:n_bytes], stable=True)
                sorted_keys = sorted_keys[:grams].contiguous()
                sorted_rows = slot_rows[:n_bytes][order[:grams]].contiguous()
                del order
            del slot_keys, slot_rows, d_text
            flags = empty(grams, torch.int64)
            _native.check(lib.crag_ngram_heads(sorted_keys.data_ptr(), sorted_rows.data_ptr(), grams, flags.data_ptr(),
                                               stream), "crag_ngram_heads")
            scan = torch.cumsum(flags[:grams], 0) if grams else flags
            last = int(scan[grams - 1]) if grams else 0
            nnz, n_terms = last & 0xFFFFFFFF, last >> 32
            d_keys, d_post_ptr = empty(n_terms, torch.int64), empty(n_terms + 1, torch.int64)
            d_post_pos, d_post_tf = empty(nnz, torch.int32), empty(nnz, torch.int16)   # (bits of the uint16 values)
            _native.check(lib.crag_ngram_emit(sorted_keys.data_ptr(), sorted_rows.data_ptr(), scan.data_ptr(), grams,
                                              n_terms, nnz, d_keys.data_ptr(), d_post_ptr.data_ptr(),
                                              d_post_pos.data_ptr(), d_post_tf.data_ptr(), scratch.data_ptr(),
                                              scratch.numel() * 8, stream), "crag_ngram_emit")
            self.keys = d_keys[:n_terms].cpu().numpy()
            self.df = np.diff(d_post_ptr[:n_terms + 1].cpu().numpy())
            self.doc_len = d_doc_len[:n].cpu().numpy()
        self.n, self.n_terms, self.nnz, self.n_grams = n, int(n_terms), int(nnz), grams
        # avgdl: fp64 sum, rounded once to fp32 (as the word lane)
        self.avgdl = float(np.float32(float(self.doc_len.sum(dtype=np.float64)) / n)) if n else 1.0
        if n and not self.avgdl > 0.0:
            self.avgdl = 1.0    # (no row holds a gram: nothing can match, the value is never used)
        self.d_keys, self.d_post_ptr, self.d_post_pos, self.d_post_tf = d_keys, d_post_ptr, d_post_pos, d_post_tf
        self.d_doc_len = d_doc_len
        self.d_ids = torch.from_numpy(self.ids if n else np.zeros(1, dtype=np.int64)).to(dev)
        self._buffers = {}

    def host_csr(self):
        """The device's inverted CSR as numpy arrays: post_ptr [V + 1] int64, post_pos [nnz] int32, post_tf [nnz] uint16."""
        return (self.d_post_ptr[:self.n_terms + 1].cpu().numpy(), self.d_post_pos[:self.nnz].cpu().numpy(),
                self.d_post_tf[:self.nnz].cpu().numpy().view(np.uint16))

    def extend(self, texts: Sequence[str], ids: Sequence[int]) -> None:
        """Rows appended at the end.  The index is rebuilt over all rows from the stored bytes (term ids are ranks among
        ALL keys, so new keys renumber the old ones anyway): its arrays equal a fresh build's.  Searches enqueued
        earlier must have finished with the old arrays (they are freed here)."""
        self.extend_bytes([(t or "").encode("utf-8", "replace") for t in texts], ids)

    def extend_bytes(self, rows_bytes: Sequence[bytes], ids: Sequence[int]) -> None:
        import torch
        self._append(rows_bytes, ids)
        torch.cuda.synchronize(self.device)
        self._build()

    def postings_bytes(self, query_texts: Sequence[str]) -> int:
        """Bytes of postings one search of these queries streams: 6 per posting of every distinct known gram."""
        _, terms, _ = self.query_terms(query_texts)
        return 6 * int(self.df[terms].sum())

    def query_terms(self, query_texts: Sequence[str]):
        """`query_terms_host` over this index's keys, df and N."""
        return query_terms_host(self.keys, self.df, self.n, query_texts)
