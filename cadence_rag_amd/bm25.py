"""BM25 lexical lane on the GPU -- the third lane of /retrieve (bm25 -> tech_tokens -> dense), which the reference
gets from Postgres + pg_search (`text @@@ :query ORDER BY pdb.score(id) DESC`, the reference's app/retrieve.py:123-180).

NOT parity with pg_search: Tantivy's arithmetic is not in the reference tree, so this is a self-defined restatement of
the published BM25 form it uses (DESIGN.md 4.7 lists the departures):

    score = sum_t qtf(t) * idf(t) * (k1 + 1) * tf / (tf + k1 * (1 - b + b * dl / avgdl)),
    idf(t) = ln(1 + (N - df + 0.5) / (df + 0.5)),  k1 = 1.2,  b = 0.75

with the statistics (N, df, dl, avgdl) of the whole index whatever the filter.  The tokeniser and the postings live
here on the host; scoring and top-k run in csrc/crag_bm25.hip behind crag_bm25_lane_host."""
from __future__ import annotations

import ctypes
import re
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native

K1 = 1.2
B = 0.75
RANGE_ROWS = 16384        # row positions per workgroup of the scoring kernel (csrc/crag_kernels.h BM25_RANGE)
MAX_QUERIES = 64
MAX_TOKEN_BYTES = 255
TF_MAX = 65535            # tf is stored in 16 bits, saturating

# [^\W_] is exactly str.isalnum() per character (the re module's \w is "isalnum() or '_'")
_RUN = re.compile(r"[^\W_]+")


def tokenize(text: str) -> List[str]:
    """Maximal runs of alphanumeric characters (str.isalnum() per character), each lower-cased; tokens longer than 255
    UTF-8 bytes are dropped.  No stemming, no stop words.  One function for rows and queries."""
    out = []
    for run in _RUN.findall(text or ""):
        tok = run.lower()
        if len(tok) <= MAX_TOKEN_BYTES // 4 or len(tok.encode("utf-8")) <= MAX_TOKEN_BYTES:
            out.append(tok)
    return out


class Bm25Index:
    """Vocabulary and per-row (term id, tf) pairs on the host, the inverted CSR on the device.

    Host (flat numpy arrays, the source of truth: `extend` appends to them and rebuilds the device side with numpy):
      vocab {token: term id}, ids handed out in order of first appearance
      row_ptr [N + 1] int64, row_terms [nnz] int32 (ascending inside a row), row_tf [nnz] int64, doc_len [N] int32
    Device: post_ptr [V + 1] int64, post_pos [nnz] int32 (row positions, ascending inside a term), post_tf [nnz] uint16,
      doc_len [N] int32, ids [N] int64."""

    def __init__(self, texts: Sequence[str], ids: Sequence[int], device) -> None:
        import torch
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.vocab: Dict[str, int] = {}
        self.row_ptr = np.zeros(1, dtype=np.int64)
        self.row_terms = np.empty(0, dtype=np.int32)
        self.row_tf = np.empty(0, dtype=np.int64)
        self.doc_len = np.empty(0, dtype=np.int32)
        self.ids = np.empty(0, dtype=np.int64)
        self._slots: dict = {}     # per stream: ring of upload slots
        self._scratch: dict = {}   # per stream: the partial top-k lists
        self._append(texts, ids)
        self._upload()

    # ---- host side ---------------------------------------------------------------------------------------------
    def _append(self, texts: Sequence[str], ids: Sequence[int]) -> None:
        new_ids = np.asarray(list(ids), dtype=np.int64).reshape(-1)
        texts = list(texts)
        if len(texts) != new_ids.size:
            raise ValueError("texts and ids must have one entry per row")
        prev = self.ids[-1] if self.ids.size else None
        if (new_ids.size and prev is not None and new_ids[0] <= prev) or np.any(np.diff(new_ids) <= 0):
            raise ValueError("ids must ascend with the row position (and continue above the stored ids)")
        if self.ids.size + new_ids.size > 2**31 - 1:
            raise ValueError("the lane addresses rows with 31 bits")
        vocab = self.vocab
        terms: List[int] = []
        tfs: List[int] = []
        lens = np.empty(len(texts), dtype=np.int64)
        dls = np.empty(len(texts), dtype=np.int32)
        for i, text in enumerate(texts):
            counts: Dict[int, int] = {}
            toks = tokenize(text)
            for tok in toks:
                t = vocab.get(tok)
                if t is None:
                    t = vocab[tok] = len(vocab)
                counts[t] = counts.get(t, 0) + 1
            row = sorted(counts.items())
            terms.extend(t for t, _ in row)
            tfs.extend(c for _, c in row)
            lens[i] = len(row)
            dls[i] = len(toks)
        self.row_ptr = np.concatenate([self.row_ptr, self.row_ptr[-1] + np.cumsum(lens)])
        self.row_terms = np.concatenate([self.row_terms, np.asarray(terms, dtype=np.int32)])
        self.row_tf = np.concatenate([self.row_tf, np.asarray(tfs, dtype=np.int64)])
        self.doc_len = np.concatenate([self.doc_len, dls])
        self.ids = np.concatenate([self.ids, new_ids])

    @classmethod
    def from_arrays(cls, row_ptr, row_terms, row_tf, n_terms: int, ids, device, vocab: Optional[Dict[str, int]] = None
                    ) -> "Bm25Index":
        """An index over rows that are (term id, tf) pairs already (a synthetic corpus, or rows tokenised elsewhere):
        row_ptr [N + 1], row_terms ascending inside a row.  `vocab` maps tokens to term ids; without one the tokens of
        a query are the decimal term ids."""
        self = cls([], [], device)
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.row_terms = np.asarray(row_terms, dtype=np.int32)
        self.row_tf = np.asarray(row_tf, dtype=np.int64)
        self.ids = np.asarray(ids, dtype=np.int64)
        if np.any(np.diff(self.ids) <= 0):
            raise ValueError("ids must ascend with the row position")
        n = self.ids.size
        self.doc_len = np.add.reduceat(np.append(self.row_tf, 0), self.row_ptr[:-1]).astype(np.int32) if n else \
            np.empty(0, dtype=np.int32)
        self.doc_len[np.diff(self.row_ptr) == 0] = 0
        self.vocab = vocab if vocab is not None else _DecimalVocab(int(n_terms))
        self._upload()
        return self

    def host_csr(self):
        """The inverted CSR as numpy arrays: post_ptr [V + 1] int64, post_pos [nnz] int32, post_tf [nnz] uint16."""
        n, v = self.ids.size, len(self.vocab)
        rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(self.row_ptr))
        order = np.argsort(self.row_terms, kind="stable")   # rows are already ascending: they stay so inside a term
        post_ptr = np.zeros(v + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.row_terms, minlength=v), out=post_ptr[1:])
        return post_ptr, rows[order], np.minimum(self.row_tf[order], TF_MAX).astype(np.uint16)

    def _upload(self) -> None:
        import torch
        post_ptr, post_pos, post_tf = self.host_csr()
        self.n = int(self.ids.size)
        self.n_terms = len(self.vocab)
        self.df = np.diff(post_ptr)
        # avgdl: fp64 sum, rounded once to fp32
        self.avgdl = float(np.float32(float(self.doc_len.sum(dtype=np.float64)) / self.n)) if self.n else 1.0
        if self.n and not self.avgdl > 0.0:
            self.avgdl = 1.0    # (no row holds a token: nothing can match, the value is never used)

        def dev(a, view=None):
            a = a if a.size else np.zeros(1, dtype=a.dtype)      # a valid address for empty arrays
            return torch.from_numpy(a.view(view) if view else a).to(self.device)
        self.d_post_ptr, self.d_post_pos = dev(post_ptr), dev(post_pos)
        self.d_post_tf = dev(post_tf, np.int16)                  # (bits of the uint16 values)
        self.d_doc_len, self.d_ids = dev(self.doc_len), dev(self.ids)
        self._scratch = {}

    def extend(self, texts: Sequence[str], ids: Sequence[int]) -> None:
        """Rows appended at the end (what the backfill does): only the new rows are tokenised; the device CSR is rebuilt
        with numpy, and N, df, avgdl -- and with them every weight -- follow.  Searches enqueued earlier must have
        finished with the old arrays (they are freed here)."""
        import torch
        self._append(texts, ids)
        torch.cuda.synchronize(self.device)
        self._upload()

    def __len__(self) -> int:
        return int(self.ids.size)

    def postings_bytes(self, query_texts: Sequence[str]) -> int:
        """Bytes of postings one search of these queries streams: 6 per posting (position + tf) of every query term."""
        total = 0
        for text in query_texts:
            total += sum(int(self.df[t]) for t in {self.vocab.get(tok) for tok in tokenize(text)} if t is not None)
        return 6 * total

    def query_terms(self, query_texts: Sequence[str]):
        """Queries -> (q_ptr int32 [nq + 1], term ids int32 ascending inside a query, weights fp32): unknown tokens are
        dropped, a token that occurs qtf times weighs qtf times (one OR clause per occurrence)."""
        q_ptr = np.zeros(len(query_texts) + 1, dtype=np.int32)
        terms: List[int] = []
        qtfs: List[int] = []
        get = self.vocab.get
        for q, text in enumerate(query_texts):
            qtf: Dict[int, int] = {}
            for tok in tokenize(text):
                t = get(tok)
                if t is not None:
                    qtf[t] = qtf.get(t, 0) + 1
            ordered = sorted(qtf)
            terms.extend(ordered)
            qtfs.extend(qtf[t] for t in ordered)
            q_ptr[q + 1] = len(terms)
        term_ids = np.asarray(terms, dtype=np.int32)
        df = self.df[term_ids].astype(np.float64)
        weights = np.asarray(qtfs, dtype=np.float64) * np.log(1.0 + (float(self.n) - df + 0.5) / (df + 0.5)) * (K1 + 1.0)
        return q_ptr, term_ids, weights.astype(np.float32)   # fp64 up to here, rounded once

    # ---- device side -------------------------------------------------------------------------------------------
    def _slot(self, stream: int):
        """Next upload slot of the stream's ring of four (the idiom of TechTokenIndex._slot)."""
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

    def search(self, query_texts: Sequence[str], k: int, row_mask=None, mask_stride: int = 0, stream: int = 0):
        """Top-k rows of every query by BM25 score (descending, equal scores by ascending id) among the rows that hold
        at least one query term and whose mask bit is set.  row_mask: packed bits per row position (uint8 CUDA tensor),
        shared (mask_stride 0) or per query.  Returns CUDA tensors ids int64 [nq, k] (-1 pad), scores fp32 [nq, k] (NaN
        pad), counts int32 [nq]; everything is enqueued on `stream` with one upload."""
        if len(query_texts) > MAX_QUERIES:
            raise ValueError("the BM25 lane takes at most 64 queries per call")
        return self.search_terms(*self.query_terms(query_texts), k, row_mask=row_mask, mask_stride=mask_stride,
                                 stream=stream)

    def search_terms(self, q_ptr, terms, weights, k: int, row_mask=None, mask_stride: int = 0, stream: int = 0):
        """`search` for queries that are term ids and weights already (the arrays of `query_terms`)."""
        import torch

        from .fusion import _on_stream
        lib = _native.load()
        nq = len(q_ptr) - 1
        if nq > MAX_QUERIES or not 1 <= int(k) <= _native.CRAG_MAX_K:
            raise ValueError(f"the BM25 lane takes at most 64 queries per call and k in [1, {_native.CRAG_MAX_K}]")
        k = int(k)
        need = int(lib.crag_bm25_scratch_bytes(self.n, max(nq, 1), k))
        with _on_stream(stream, self.device):
            scratch = self._scratch.get(stream)
            if scratch is None or scratch.numel() * 8 < need:
                # sized for a full batch at this k, so that a stream allocates once
                full = int(lib.crag_bm25_scratch_bytes(self.n, MAX_QUERIES, k))
                scratch = self._scratch[stream] = torch.empty((max(need, full) + 7) // 8, dtype=torch.int64,
                                                              device=self.device)
            out_ids = torch.empty(nq, k, dtype=torch.int64, device=self.device)
            out_scores = torch.empty(nq, k, dtype=torch.float32, device=self.device)
            out_counts = torch.empty(nq, dtype=torch.int32, device=self.device)
        if nq == 0:
            return out_ids, out_scores, out_counts
        rc = lib.crag_bm25_lane_host(
            self.d_post_ptr.data_ptr(), self.d_post_pos.data_ptr(), self.d_post_tf.data_ptr(), self.d_doc_len.data_ptr(),
            self.d_ids.data_ptr(), self.n, self.n_terms, ctypes.c_float(self.avgdl),
            q_ptr.ctypes.data, terms.ctypes.data if terms.size else None, weights.ctypes.data if weights.size else None,
            nq, k, None if row_mask is None else row_mask.data_ptr(), int(mask_stride), self._slot(stream),
            scratch.data_ptr(), scratch.numel() * 8, out_ids.data_ptr(), out_scores.data_ptr(), out_counts.data_ptr(),
            ctypes.c_void_p(stream))
        _native.check(rc, "crag_bm25_lane_host")
        return out_ids, out_scores, out_counts


class _DecimalVocab:
    """Vocabulary of an index built from term ids (Bm25Index.from_arrays): token "17" is term 17."""

    def __init__(self, n_terms: int) -> None:
        self.n_terms = n_terms

    def __len__(self) -> int:
        return self.n_terms

    def get(self, tok, default=None):
        try:
            t = int(tok)
        except ValueError:
            return default
        return t if 0 <= t < self.n_terms else default
